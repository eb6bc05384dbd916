"""Measurement of paged KV-cache attention (include/flashattn_amd_paged.h): writes profiles/kv_paged.txt and docs/kv_paged.md.

    python profiles/kv_paged.py [--out-dir DIR]          # GPU: one run (about a minute)
    python profiles/kv_paged.py --trace-shape 512,8192    # GPU, for `rocprofv3 --kernel-trace --stats -- python ...`: arm a and the page-16 arms only

Shapes: d = 128, nq = 1, group 8, bf16 output, bh_kv x nk in {8 x 8192, 64 x 8192, 512 x 2048, 512 x 8192}.
The timing method is profiles/kv_decode.py's: device events around 200 warmed launches on one stream, rotating over enough distinct K/V buffers
that the footprint exceeds the 256 MB Infinity Cache, arms alternated, three repeats, medians; the spread of an arm is (max - min) / median.
Arms per shape:
  a  fa_kv_forward on the contiguous cache (bh_kv, nk, d)              b  fa_kv_stream_read on the same buffers (the floor)
  p  fa_paged_forward on THE SAME MEMORY seen as a pool (bh_kv * nk / page, page, d), one sequence per slab, pages of 16, 64 and 256 rows, with
     an identity table (sequence b, page p -> b * nk / page + p: the contiguous cache, found through the table) and a shuffled table (one
     random permutation of all pages of the buffer: every sequence's pages lie anywhere in it).  The same bytes as arm a in every case.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, GROUP = 128, 8
SHAPES = [(8, 8192), (64, 8192), (512, 2048), (512, 8192)]
PAGES = (16, 64, 256)
LAUNCHES, REPEATS = 200, 3
ROTATE_BYTES = 1 << 30            # K + V over all rotated buffers: four times the Infinity Cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None, help="write kv_paged.txt / kv_paged.md here instead of profiles/ and docs/")
    ap.add_argument("--trace-shape", default=None, help="bh_kv,nk: run arm a and the page-16 arms 50 times each and exit (for rocprofv3)")
    ap.add_argument("--quick", action="store_true", help="rehearsal: the first shape, 20 launches")
    a = ap.parse_args()

    import torch
    from flashattention_c_amd import _cabi_kv, _cabi_paged
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    BF16 = _cabi_kv.FA_DTYPE_BF16
    KV, PG = _cabi_kv.lib(), _cabi_paged.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    class Case:
        """the buffers of one shape: nbuf rotated K/V caches, q / o / workspace, and the block tables that see a cache as a pool"""

        def __init__(self, bh, nk):
            self.bh, self.nk = bh, nk
            self.kv_bytes = 2 * bh * nk * D * 2
            self.nbuf = max(1, -(-ROTATE_BYTES // self.kv_bytes))
            self.k = torch.empty(self.nbuf, bh, nk, D, dtype=torch.bfloat16, device=dev).normal_()
            self.v = torch.empty(self.nbuf, bh, nk, D, dtype=torch.bfloat16, device=dev).normal_()
            self.q = torch.randn(bh * GROUP, 1, D, device=dev).to(torch.bfloat16)
            self.o = torch.empty(bh * GROUP, 1, D, dtype=torch.bfloat16, device=dev)
            self.sink = torch.zeros(1024, dtype=torch.int32, device=dev)
            need = int(KV.fa_kv_workspace_bytes(bh, GROUP, 1, nk, D, 0, BF16))
            assert need == int(PG.fa_paged_workspace_bytes(bh, 1, GROUP, 1, nk, D, 0, BF16))
            self.ws, self.need = torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need
            self.tables = {}
            gen = torch.Generator().manual_seed(bh * 131 + nk)
            for page in PAGES:
                n = bh * nk // page
                ident = torch.arange(n, dtype=torch.int32)
                self.tables[page, "identity"] = ident.view(bh, nk // page).to(dev)
                self.tables[page, "shuffled"] = ident[torch.randperm(n, generator=gen)].view(bh, nk // page).contiguous().to(dev)
            # the cache descriptors, built once: the timed loop of a paged arm does the host work of arm a's, one foreign call per launch
            self.caches = {(page, kind, j): _cabi_paged.FaPagedCache(self.k[j].data_ptr(), self.v[j].data_ptr(), bh * nk // page, page, page * D, D, 0,
                                                                     t.data_ptr(), nk // page, None)
                           for (page, kind), t in self.tables.items() for j in range(self.nbuf)}

        def forward(self, i):
            j = i % self.nbuf
            rc = KV.fa_kv_forward(self.q.data_ptr(), self.k[j].data_ptr(), self.v[j].data_ptr(), self.o.data_ptr(), None, self.bh, GROUP, 1, self.nk, self.nk,
                                  None, D, 0.088, 0, BF16, self.ws.data_ptr() if self.need else None, self.need, stream())
            assert rc == 0, KV.fa_kv_last_error()

        def paged(self, page, kind, i):
            rc = PG.fa_paged_forward(self.q.data_ptr(), ctypes.byref(self.caches[page, kind, i % self.nbuf]), self.o.data_ptr(), None, self.bh, 1, GROUP, 1, self.nk, D, 0.088, 0, BF16,
                                     self.ws.data_ptr() if self.need else None, self.need, stream())
            assert rc == 0, PG.fa_paged_last_error()

        def stream_read(self, i):
            j = i % self.nbuf
            assert KV.fa_kv_stream_read(self.k[j].data_ptr(), self.v[j].data_ptr(), self.bh, self.nk, self.nk, D, self.sink.data_ptr(), stream()) == 0

        def check(self):
            """every paged arm computes what fa_kv_forward computes on the cache its table describes -- buffer 0 itself under an identity table,
            a gathered copy under a shuffled one -- to the bit (the same plan, the same operation sequence)"""
            for (page, kind), t in self.tables.items():
                kc, vc = (x[0].view(-1, page, D)[t.long()].reshape(self.bh, self.nk, D) for x in (self.k, self.v))
                rc = KV.fa_kv_forward(self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), self.o.data_ptr(), None, self.bh, GROUP, 1, self.nk, self.nk,
                                      None, D, 0.088, 0, BF16, self.ws.data_ptr() if self.need else None, self.need, stream())
                assert rc == 0, KV.fa_kv_last_error()
                want = self.o.clone()
                self.o.zero_()
                self.paged(page, kind, 0)
                assert torch.equal(self.o.view(torch.int16), want.view(torch.int16)), (page, kind)
                del kc, vc

    def timed(fn, launches):
        """microseconds per launch: device events around `launches` launches on the current stream, after a tenth as many warm-ups"""
        for i in range(max(2, launches // 10)):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(launches):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    if a.trace_shape:
        bh, nk = map(int, a.trace_shape.split(","))
        c = Case(bh, nk)
        timed(c.forward, 50)
        timed(lambda i: c.paged(16, "identity", i), 50)
        timed(lambda i: c.paged(16, "shuffled", i), 50)
        return

    shapes = SHAPES[:1] if a.quick else SHAPES
    launches = 20 if a.quick else LAUNCHES
    free, _ = torch.cuda.mem_get_info()
    say(f"# {PG.fa_paged_version().decode()}; {torch.cuda.get_device_name(0)}; {launches} launches per timing, {REPEATS} repeats (median; spread = (max - min) / median)")
    say()
    say("us per launch; p / a in brackets.  d = 128, nq = 1, group 8, bf16 output; every paged arm reads the buffers of arm a through a block table and was")
    say("checked, before it was timed, to give bit for bit what fa_kv_forward gives on the cache its table describes.")
    say()
    heads = [f"p{page} {kind}" for page in PAGES for kind in ("identity", "shuffled")]
    say("| bh_kv x nk | K+V MB | buffers | S | a: fa_kv_forward | a GB/s | a spread | b: stream read | a / b | " + " | ".join(heads) + " |")
    say("|---|---|---|---|---|---|---|---|---|" + "---|" * len(heads))
    beyond = []
    for bh, nk in shapes:
        kv = 2 * bh * nk * D * 2
        if 2.5 * max(kv, ROTATE_BYTES) > free:
            say(f"| {bh} x {nk} | {kv / 2**20:.0f} | skipped: K + V exceed the free memory |")
            continue
        c = Case(bh, nk)
        c.check()
        S = KV.fa_kv_splits_for(bh, GROUP, 1, nk, D, 0, BF16)
        assert S == PG.fa_paged_splits_for(bh, 1, GROUP, 1, nk, D, 0, BF16)
        arms = {"a": c.forward, "b": c.stream_read}
        for page in PAGES:
            for kind in ("identity", "shuffled"):
                arms[f"p{page} {kind}"] = lambda i, page=page, kind=kind: c.paged(page, kind, i)
        t = {k: [] for k in arms}
        for _ in range(REPEATS):
            for k, fn in arms.items():
                t[k].append(timed(fn, launches))
        med = {k: statistics.median(x) for k, x in t.items()}
        spread = {k: (max(x) - min(x)) / statistics.median(x) for k, x in t.items()}
        say(f"| {bh} x {nk} | {kv / 2**20:.0f} | {c.nbuf} | {S} | {med['a']:.1f} | {kv / med['a'] / 1e3:.0f} | {100 * spread['a']:.1f} % | {med['b']:.1f} | {med['a'] / med['b']:.2f} | "
            + " | ".join(f"{med[h]:.1f} ({med[h] / med['a']:.3f})" for h in heads) + " |")
        for h in heads:
            if med[h] / med["a"] - 1.0 > spread["a"]:
                beyond.append(f"{bh} x {nk} {h}: {med[h] / med['a']:.3f} (a's spread {100 * spread['a']:.1f} %, the arm's own {100 * spread[h]:.1f} %)")
        del c, arms
        torch.cuda.empty_cache()
    say()
    say("p / a beyond the spread of arm a's own repeats: " + ("; ".join(beyond) or "none"))

    # profiles/kv_paged.txt: the run as printed; docs/kv_paged.md: the same tables between the two markers, the prose around them is kept
    out_txt = os.path.join(a.out_dir or os.path.join(ROOT, "profiles"), "kv_paged.txt")
    out_md = os.path.join(a.out_dir or os.path.join(ROOT, "docs"), "kv_paged.md")
    os.makedirs(os.path.dirname(out_txt), exist_ok=True)
    body = "\n".join(lines) + "\n"
    with open(out_txt, "w") as f:
        f.write(body)
    begin, end = "<!-- measured:begin -->\n", "<!-- measured:end -->\n"
    doc = os.path.join(ROOT, "docs", "kv_paged.md")
    text = open(doc).read() if os.path.exists(doc) else f"# Paged KV-cache attention: measurements\n\n{begin}{end}"
    head, rest = text.split(begin)
    with open(out_md, "w") as f:
        f.write(head + begin + body + end + rest.split(end)[1])


if __name__ == "__main__":
    main()
