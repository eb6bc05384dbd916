"""CPU: every check of the KV-cache libraries' host side (csrc/fa_kv_host.h behind fa_kv_plan.cpp, fa_paged_host.cpp, fa_kv8_host.cpp), one bad
call each, over the four *_forward entries, fa_kv_stream_read and the *_workspace_bytes / *_splits_for / *_kernel_name_for queries: the return
code AND the text of *_last_error() against tests/golden/kv_host_errors.txt, recorded from the commit before the three validators became one.
The order of the checks is held with it: most calls break one thing, and the ones that break two name the check that must answer first.

No call here reaches a launch (each forward row is asserted to end in FA_ERR_INVALID_ARGUMENT or FA_ERR_UNSUPPORTED), so no device is
touched and no pointer dereferenced.

Re-record (after a change that is MEANT to move a message or a code):
    python flashattention.c_amd/build.py && python -m tests.test_kv_host_errors --record
"""
import ctypes
import os
import sys

from flashattention_c_amd import _cabi_kv, _cabi_kv8, _cabi_paged
from tests.conftest import GOLDEN_DIR

GOLDEN = os.path.join(GOLDEN_DIR, "kv_host_errors.txt")
BF16, BF16_F32, F32 = _cabi_kv.FA_DTYPE_BF16, _cabi_kv.FA_DTYPE_BF16_OUT_F32, _cabi_kv.FA_DTYPE_F32
A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call
G = 1 << 30
NAN, INF = float("nan"), float("inf")

# what breaks check_shape, by the entry's own argument names (B: the slab count -- bh_kv, or batch where the entry has heads_kv)
SHAPE = [dict(B=0), dict(group=0), dict(nq=0), dict(nk=0), dict(dtype=F32), dict(dtype=7), dict(d=96), dict(d=32),
         dict(nk=(1 << 24) + 1, cap=(1 << 24) + 1, d=64, page_size=65536, max_pages=512),
         dict(nq=(1 << 30) + 1), dict(group=1 << 16, nq=1 << 15), dict(B=1 << 31), dict(B=1 << 29, group=4),
         dict(B=1 << 20, group=1, nq=1 << 20)]
SHAPE_PAGED = [dict(heads_kv=0), dict(B=1 << 16, heads_kv=1 << 15), dict(B=1 << 14, heads_kv=1 << 15, group=4)]
SCALES = [dict(scale=0.0), dict(scale=NAN), dict(scale=INF)]
SCALES8 = [dict(k_scale=s) for s in (0.0, -1.0, INF, NAN)] + [dict(v_scale=s) for s in (0.0, -1.0, INF, NAN)] + \
          [dict(scale=1e30, k_scale=1e30), dict(scale=1e-30, k_scale=1e-30)]


def _only(kw, names):
    return {k: v for k, v in kw.items() if k in names}


# ---- contiguous: fa_kv_forward (2-byte elements), fa_kv8_forward (1 byte) ----
Q, K, V, O, LSE, LENS, WS = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 4 * G, A + 4 * G + (1 << 20), A + 5 * G


def contiguous(L, fp8, **kw):
    a = dict(q=Q, k=K, v=V, o=O, lse=None, B=2, group=4, nq=1, nk=4096, cap=4096, lens=None, d=128, scale=1.0, k_scale=0.5, v_scale=2.0, causal=0,
             dtype=BF16, ws=None, ws_bytes=0)
    a.update(_only(kw, a))
    head = (a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["group"], a["nq"], a["nk"], a["cap"], a["lens"], a["d"], a["scale"])
    tail = (a["causal"], a["dtype"], a["ws"], a["ws_bytes"], None)
    if fp8:
        return L.fa_kv8_forward(*head, a["k_scale"], a["v_scale"], *tail)
    return L.fa_kv_forward(*head, *tail)


def contiguous_cases(es, need):
    slab, rows = 4096 * 128 * es, 2 * 4 * 1
    return [dict(q=None), dict(k=None), dict(v=None), dict(o=None), *SHAPE,
            dict(nk=4097), dict(cap=(1 << 25) // es), *SCALES, *(SCALES8 if es == 1 else []),
            dict(q=Q + 8), dict(k=K + 8), dict(v=V + 8), dict(o=O + 8), dict(lse=LSE + 2), dict(lens=LENS + 1), dict(ws=WS + 128, ws_bytes=need),
            dict(o=Q), dict(nk=100, o=K + slab + 4000 * 128 * es), dict(nk=100, o=V + 2 * slab - 16),
            dict(lse=Q + 4), dict(lse=K + slab), dict(lse=V + 2 * slab - 4), dict(lse=O + rows * 128 * 2 - 4),
            dict(ws=WS, ws_bytes=need - 1), dict(ws=WS, ws_bytes=1),
            dict(ws=Q, ws_bytes=need), dict(ws=K + 2 * slab - 256, ws_bytes=need), dict(ws=V, ws_bytes=need), dict(ws=O, ws_bytes=need),
            dict(lse=WS + 256, ws=WS, ws_bytes=need), dict(lens=WS + 512, ws=WS, ws_bytes=need)]


# ---- paged: fa_paged_forward, fa_kv8_paged_forward.  2 sequences x 2 heads, (pages, page, H, d) pools of 64 pages of 64 rows ----
POOL_K, POOL_V, TABLE, LENS_P, OP, LSE_P = A + 1 * G, A + 2 * G, A + 3 * G, A + 3 * G + (1 << 20), A + 4 * G, A + 6 * G


def paged(L, fp8, **kw):
    a = dict(q=Q, o=OP, lse=None, cache=True, B=2, heads_kv=2, group=4, nq=1, nk=2048, d=128, scale=1.0, k_scale=0.5, v_scale=2.0, causal=0, dtype=BF16,
             ws=None, ws_bytes=0)
    f = dict(k_pool=POOL_K, v_pool=POOL_V, num_pages=64, page_size=64, page_stride=64 * 2 * 128, row_stride=2 * 128, head_stride=128, block_table=TABLE,
             max_pages=32, seq_lens=LENS_P)
    a.update(_only(kw, a))
    f.update(_only(kw, f))
    cache = ctypes.byref(_cabi_paged.FaPagedCache(**f)) if a["cache"] else None
    head = (a["q"], cache, a["o"], a["lse"], a["B"], a["heads_kv"], a["group"], a["nq"], a["nk"], a["d"], a["scale"])
    tail = (a["causal"], a["dtype"], a["ws"], a["ws_bytes"], None)
    if fp8:
        return L.fa_kv8_paged_forward(*head, a["k_scale"], a["v_scale"], *tail)
    return L.fa_paged_forward(*head, *tail)


def paged_cases(es, need):
    page_bytes, o_bytes = 64 * 2 * 128 * es, 2 * 2 * 4 * 128 * 2
    big = dict(page_size=65536, max_pages=1, page_stride=(1 << 32) // es)   # 2^32 bytes inside a page: by the rows, by the head offset
    return [dict(q=None), dict(o=None), dict(cache=False), dict(k_pool=None), dict(v_pool=None), dict(block_table=None), *SHAPE, *SHAPE_PAGED,
            dict(page_size=8), dict(page_size=24), dict(page_size=1 << 17, max_pages=1, row_stride=128, head_stride=0, heads_kv=1), dict(page_size=-16),
            dict(num_pages=0), dict(num_pages=1 << 31), dict(max_pages=0), dict(nk=2049),
            dict(page_stride=12), dict(row_stride=2 * 128 + 12), dict(head_stride=12),
            *([dict(page_stride=64 * 2 * 128 + 8), dict(row_stride=2 * 128 + 8), dict(head_stride=128 + 8)] if es == 1 else []),   # 8 elements: 8 bytes
            dict(row_stride=64, heads_kv=1, head_stride=0), dict(page_stride=0), dict(head_stride=-16),
            dict(page_stride=(1 << 40) + 16), dict(head_stride=(1 << 40) + 16), dict(row_stride=(1 << 40) + 16),
            dict(big, row_stride=65536 // es, heads_kv=1, head_stride=0, B=4), dict(big, row_stride=(65536 - 16) // es, heads_kv=2, head_stride=65536 * 16 // es),
            *SCALES, *(SCALES8 if es == 1 else []),
            dict(q=Q + 8), dict(o=OP + 8), dict(k_pool=POOL_K + 8), dict(v_pool=POOL_V + 8), dict(lse=LSE_P + 2), dict(block_table=TABLE + 2),
            dict(seq_lens=LENS_P + 1), dict(ws=WS + 128, ws_bytes=need),
            dict(o=Q), dict(o=POOL_K + 40 * page_bytes), dict(o=POOL_V + 63 * page_bytes + 1024), dict(o=TABLE), dict(o=LENS_P),
            dict(lse=Q + 4), dict(lse=POOL_K + 63 * page_bytes), dict(lse=POOL_V + 5 * page_bytes), dict(lse=TABLE + 4), dict(lse=LENS_P + 4),
            dict(lse=OP + o_bytes - 4),
            dict(ws=WS, ws_bytes=need - 1), dict(ws=WS, ws_bytes=1),
            dict(ws=Q, ws_bytes=need), dict(ws=POOL_K + 63 * page_bytes, ws_bytes=need), dict(ws=POOL_V, ws_bytes=need), dict(ws=TABLE, ws_bytes=need),
            dict(ws=TABLE + 256, ws_bytes=need, max_pages=4096), dict(ws=LENS_P - 256, ws_bytes=need), dict(ws=OP, ws_bytes=need),
            dict(lse=WS + 256, ws=WS, ws_bytes=need)]


def _label(kw):
    return " ".join(f"{k}={v:#x}" if isinstance(v, int) and abs(v) >= 4096 else f"{k}={v}" for k, v in kw.items()) or "-"


def _text(b):
    return (b or b"").decode()


def walk():
    """[(label, outcome, message)] over the three libraries, in a fixed order"""
    rows = []
    KV, PG, K8 = _cabi_kv.lib(), _cabi_paged.lib(), _cabi_kv8.lib()

    def forwards(entry, call, L, fp8, cases, last_error):
        for kw in cases:
            rc = call(L, fp8, **kw)
            assert rc in (1, 2), (entry, kw, rc, last_error())   # a call that passes validation would launch
            rows.append((f"{entry} {_label(kw)}", str(rc), _text(last_error())))

    def queries(lib_tag, L, prefix, shape_args, last_error, pages):
        """the shape queries on a good shape and on each bad one; kernel_name_for over page sizes where it takes one"""
        good = dict(B=2, heads_kv=2, group=4, nq=1, nk=4096, d=128, causal=1, dtype=BF16_F32)
        for kw in [{}] + SHAPE + (SHAPE_PAGED if "heads_kv" in shape_args else []):
            a = dict(good, **_only(kw, good))
            args = [a[n] for n in shape_args]
            ws, S = getattr(L, prefix + "workspace_bytes")(*args), getattr(L, prefix + "splits_for")(*args)
            for page in pages:
                name = getattr(L, prefix + "kernel_name_for")(*args, *([] if page is None else [page]))
                msg = _text(last_error()) if name is None else ""   # a query that succeeds leaves the message alone
                rows.append((f"{lib_tag} queries {_label(kw)} page={page}", f"{ws},{S},{_text(name) or None}", msg))

    need = KV.fa_kv_workspace_bytes(2, 4, 1, 4096, 128, 0, BF16)
    forwards("fa_kv_forward", contiguous, KV, False, contiguous_cases(2, need), KV.fa_kv_last_error)
    for kw in (dict(k=None), dict(v=None), dict(sink=None), dict(B=0), dict(nk=0), dict(d=96), dict(nk=4097), dict(cap=1 << 24), dict(k=K + 8), dict(sink=WS + 4)):
        a = dict(k=K, v=V, B=2, nk=4096, cap=4096, d=128, sink=WS)
        a.update(kw)
        rc = KV.fa_kv_stream_read(a["k"], a["v"], a["B"], a["nk"], a["cap"], a["d"], a["sink"], None)
        assert rc in (1, 2), (kw, rc)
        rows.append((f"fa_kv_stream_read {_label(kw)}", str(rc), _text(KV.fa_kv_last_error())))
    queries("kv", KV, "fa_kv_", ("B", "group", "nq", "nk", "d", "causal", "dtype"), KV.fa_kv_last_error, (None,))

    need = PG.fa_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 0, BF16)
    forwards("fa_paged_forward", paged, PG, False, paged_cases(2, need), PG.fa_paged_last_error)
    queries("paged", PG, "fa_paged_", ("B", "heads_kv", "group", "nq", "nk", "d", "causal", "dtype"), PG.fa_paged_last_error, (16, 65536, 0, 8, 24, 1 << 17, -16))

    need = K8.fa_kv8_workspace_bytes(2, 4, 1, 4096, 128, 0, BF16)
    forwards("fa_kv8_forward", contiguous, K8, True, contiguous_cases(1, need), K8.fa_kv8_last_error)
    need = K8.fa_kv8_workspace_bytes(4, 4, 1, 2048, 128, 0, BF16)
    forwards("fa_kv8_paged_forward", paged, K8, True, paged_cases(1, need), K8.fa_kv8_last_error)
    queries("kv8", K8, "fa_kv8_", ("B", "group", "nq", "nk", "d", "causal", "dtype"), K8.fa_kv8_last_error, (0, 16, 65536, 8, 24, 1 << 17, -16))
    assert len({r[0] for r in rows}) == len(rows)
    return rows


def test_every_check_answers_with_the_recorded_code_and_message():
    want = [tuple(ln.split("\t")) for ln in open(GOLDEN).read().splitlines() if ln and not ln.startswith("#")]
    have = walk()
    assert [r[0] for r in have] == [r[0] for r in want]
    assert len(have) > 300
    diff = [f"{h[0]}\n    recorded: {w[1:]}\n    now:      {h[1:]}" for h, w in zip(have, want) if h != w]
    assert not diff, "\n".join(diff)
    # every message of a failed forward says something, and the table reaches both kinds of failure in every entry
    for entry in ("fa_kv_forward", "fa_paged_forward", "fa_kv8_forward", "fa_kv8_paged_forward"):
        mine = [r for r in have if r[0].startswith(entry + " ")]
        assert {r[1] for r in mine} == {"1", "2"} and all(r[2] for r in mine), entry


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    rows = walk()
    assert not any("\t" in f or "\n" in f for r in rows for f in r)
    with open(GOLDEN, "w") as f:
        f.write("# (return code or query results, *_last_error() text) of every bad call tests/test_kv_host_errors.py makes, tab-separated.\n"
                "# Re-record: python flashattention.c_amd/build.py && python -m tests.test_kv_host_errors --record\n")
        for r in rows:
            f.write("\t".join(r) + "\n")
    print(f"{len(rows)} calls -> {GOLDEN}")
