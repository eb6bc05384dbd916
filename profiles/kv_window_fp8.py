"""Measurement of sliding-window KV-cache attention over an fp8 cache (include/flashattn_amd_kvw8.h): writes profiles/kv_window_fp8.txt and the
marked block of docs/kv_window_fp8.md.  profiles/kv_window.py for the fp8 libraries.

    python profiles/kv_window_fp8.py [--out-dir DIR]          # GPU: one run (a few minutes)

The question: does a windowed fp8 call over a long cache cost what fa_kv8_forward costs on a cache of W keys, whatever the length is?
Shapes: d = 128, nq = 1, group 8, causal, bf16 output, window_left = 4095 (W = 4096 keys), bh_kv in {8, 64, 512, 1024}; K/V are random e4m3 bytes
without NaN codes (bit 6 cleared, as in profiles/kv_fp8.py), k_scale = v_scale = 1.
The timing method is profiles/kv_decode.py's: device events around 200 warmed launches on one stream, rotating over enough distinct K/V buffers
that the bytes the WINDOW touches exceed four times the 256 MB Infinity Cache, arms alternated, three repeats, medians; the spread of an arm is
(max - min) / median of its three repeats.
Arms per bh_kv, all on the same buffers (slabs of 33024 rows):
  a  fa_kvw8_forward at len 8192 and 32768 (len - 4096 a multiple of 64: the window starts at a block boundary) and at len 8193 and 32769
     (len - 4096 = 1 mod 64: up to 63 alignment keys more)
  b  fa_kv8_forward (the unwindowed fp8 library, unchanged) at nk = 4096 on the same slabs: the same number of keys
  c  fa_kv8_forward over the full len: what a caller paid before, for the wrong answer
  the same through the paged entries at pages of 16 and 256 rows (identity tables over the same memory): fa_kvw8_paged_forward against
  fa_kv8_paged_forward at nk = 4096.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, GROUP, WINDOW_LEFT = 128, 8, 4095
W = WINDOW_LEFT + 1
BHS = (8, 64, 512, 1024)
LENS = (8192, 8193, 32768, 32769)
PAGES = (16, 256)
CAP = 32768 + 256                 # rows per slab: holds len 32769, a whole number of 256-row pages
LAUNCHES, REPEATS = 200, 3
ROTATE_BYTES = 1 << 30            # K + V rows inside the window over all rotated buffers: four times the Infinity Cache
SCALE = 0.088


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None, help="write kv_window_fp8.txt / kv_window_fp8.md here instead of profiles/ and docs/")
    ap.add_argument("--quick", action="store_true", help="rehearsal: the first bh_kv, 20 launches")
    a = ap.parse_args()

    import torch
    from flashattention_c_amd import _cabi_kv8, _cabi_kvw8, _cabi_paged
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    BF16 = _cabi_kv8.FA_DTYPE_BF16
    KV, KW = _cabi_kv8.lib(), _cabi_kvw8.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    class Case:
        """the buffers of one bh_kv: nbuf rotated K/V caches of CAP rows per slab, q / o / workspace, identity block tables"""

        def __init__(self, bh):
            self.bh = bh
            self.win_bytes = 2 * bh * W * D
            self.nbuf = max(1, -(-ROTATE_BYTES // self.win_bytes))
            self.k, self.v = (torch.randint(0, 256, (self.nbuf, bh, CAP, D), dtype=torch.uint8, device=dev) & 0xBF for _ in range(2))
            self.q = torch.randn(bh * GROUP, 1, D, device=dev).to(torch.bfloat16)
            self.o = torch.empty(bh * GROUP, 1, D, dtype=torch.bfloat16, device=dev)
            needs = [int(KW.fa_kvw8_workspace_bytes(bh, GROUP, 1, n, D, 1, BF16, WINDOW_LEFT)) for n in LENS]
            needs += [int(KV.fa_kv8_workspace_bytes(bh, GROUP, 1, n, D, 1, BF16)) for n in (W,) + LENS]
            self.ws = torch.empty(max(needs + [256]), dtype=torch.uint8, device=dev)
            self.tables = {page: torch.arange(bh * CAP // page, dtype=torch.int32).view(bh, CAP // page).to(dev) for page in PAGES}
            self.caches = {(page, j): _cabi_paged.FaPagedCache(self.k[j].data_ptr(), self.v[j].data_ptr(), bh * CAP // page, page, page * D, D, 0,
                                                               t.data_ptr(), CAP // page, None)
                           for page, t in self.tables.items() for j in range(self.nbuf)}

        def _ws(self, need):
            return (self.ws.data_ptr() if need else None), need

        def windowed(self, n, i, o=None):
            j = i % self.nbuf
            rc = KW.fa_kvw8_forward(self.q.data_ptr(), self.k[j].data_ptr(), self.v[j].data_ptr(), (o if o is not None else self.o).data_ptr(), None, self.bh, GROUP, 1,
                                    n, CAP, None, D, SCALE, 1.0, 1.0, 1, BF16, WINDOW_LEFT,
                                    *self._ws(int(KW.fa_kvw8_workspace_bytes(self.bh, GROUP, 1, n, D, 1, BF16, WINDOW_LEFT))), stream())
            assert rc == 0, KW.fa_kvw8_last_error()

        def plain(self, n, i):
            j = i % self.nbuf
            rc = KV.fa_kv8_forward(self.q.data_ptr(), self.k[j].data_ptr(), self.v[j].data_ptr(), self.o.data_ptr(), None, self.bh, GROUP, 1, n, CAP, None, D, SCALE,
                                   1.0, 1.0, 1, BF16, *self._ws(int(KV.fa_kv8_workspace_bytes(self.bh, GROUP, 1, n, D, 1, BF16))), stream())
            assert rc == 0, KV.fa_kv8_last_error()

        def windowed_paged(self, page, n, i, o=None):
            rc = KW.fa_kvw8_paged_forward(self.q.data_ptr(), ctypes.byref(self.caches[page, i % self.nbuf]), (o if o is not None else self.o).data_ptr(), None, self.bh, 1,
                                          GROUP, 1, n, D, SCALE, 1.0, 1.0, 1, BF16, WINDOW_LEFT,
                                          *self._ws(int(KW.fa_kvw8_paged_workspace_bytes(self.bh, 1, GROUP, 1, n, D, 1, BF16, WINDOW_LEFT))), stream())
            assert rc == 0, KW.fa_kvw8_last_error()

        def plain_paged(self, page, n, i):
            rc = KV.fa_kv8_paged_forward(self.q.data_ptr(), ctypes.byref(self.caches[page, i % self.nbuf]), self.o.data_ptr(), None, self.bh, 1, GROUP, 1, n, D, SCALE,
                                         1.0, 1.0, 1, BF16, *self._ws(int(KV.fa_kv8_workspace_bytes(self.bh, GROUP, 1, n, D, 1, BF16))), stream())
            assert rc == 0, KV.fa_kv8_last_error()

        def check(self):
            """every windowed arm against fa_kv8_forward on a copy of the window's rows of buffer 0 (another plan: close, not the same bits), and
            the paged windowed arms against the contiguous one, bit for bit"""
            for n in LENS:
                kc, vc = (x[0][:, n - W:n].contiguous() for x in (self.k, self.v))
                want = torch.empty_like(self.o)
                rc = KV.fa_kv8_forward(self.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), want.data_ptr(), None, self.bh, GROUP, 1, W, W, None, D, SCALE, 1.0, 1.0, 1, BF16,
                                       *self._ws(int(KV.fa_kv8_workspace_bytes(self.bh, GROUP, 1, W, D, 1, BF16))), stream())
                assert rc == 0, KV.fa_kv8_last_error()
                got = torch.empty_like(self.o)
                self.windowed(n, 0, got)
                assert float((got.float() - want.float()).abs().max()) < 2e-3, (self.bh, n)
                for page in PAGES:
                    gp = torch.empty_like(self.o)
                    self.windowed_paged(page, n, 0, gp)
                    assert torch.equal(gp.view(torch.int16), got.view(torch.int16)), (self.bh, n, page)
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

    bhs = BHS[:1] if a.quick else BHS
    launches = 20 if a.quick else LAUNCHES
    free, _ = torch.cuda.mem_get_info()
    say(f"# {KW.fa_kvw8_version().decode()}; {torch.cuda.get_device_name(0)}; {launches} launches per timing, {REPEATS} repeats (median; spread = (max - min) / median)")
    say()
    say(f"us per launch.  d = {D}, nq = 1, group {GROUP}, causal, bf16 output, e4m3 K/V, window_left = {WINDOW_LEFT}.  a: the windowed call at this len; b: the unwindowed call on")
    say(f"{W} keys of the same slabs; c: the unwindowed call over the full len.  allowed: b's spread, plus 63 / 4096 = 1.5 % where len - 4096 is no multiple of 64.")
    say()
    say("| entry | bh_kv | len | buffers | S a | S b | a us | b us | b spread | a / b | allowed | c us | a / c |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    beyond, by_len = [], []
    for bh in bhs:
        if 2.5 * 2 * bh * CAP * D > free:
            say(f"| all | {bh} | skipped: K + V exceed the free memory |")
            continue
        c = Case(bh)
        c.check()
        for entry in ("contiguous",) + tuple(f"paged {p}" for p in PAGES):
            page = int(entry.split()[1]) if entry != "contiguous" else None
            arms = {}
            for n in LENS:
                arms["a", n] = (lambda i, n=n: c.windowed(n, i)) if page is None else (lambda i, n=n: c.windowed_paged(page, n, i))
            arms["b", W] = (lambda i: c.plain(W, i)) if page is None else (lambda i: c.plain_paged(page, W, i))
            for n in (8192, 32768):
                arms["c", n] = (lambda i, n=n: c.plain(n, i)) if page is None else (lambda i, n=n: c.plain_paged(page, n, i))
            t = {k: [] for k in arms}
            for _ in range(REPEATS):
                for k, fn in arms.items():
                    t[k].append(timed(fn, launches))
            med = {k: statistics.median(x) for k, x in t.items()}
            b, spread_b = med["b", W], (max(t["b", W]) - min(t["b", W])) / med["b", W]
            Sb = KV.fa_kv8_splits_for(bh, GROUP, 1, W, D, 1, BF16)
            for n in LENS:
                Sa = KW.fa_kvw8_splits_for(bh, GROUP, 1, n, D, 1, BF16, WINDOW_LEFT)
                allowed = spread_b + (63 / 4096 if (n - W) % 64 else 0.0)
                cn = med["c", n - (n - W) % 64]
                say(f"| {entry} | {bh} | {n} | {c.nbuf} | {Sa} | {Sb} | {med['a', n]:.1f} | {b:.1f} | {100 * spread_b:.1f} % | {med['a', n] / b:.3f} | {100 * allowed:.1f} % | "
                    f"{cn:.1f} | {med['a', n] / cn:.3f} |")
                if med["a", n] / b - 1.0 > allowed:
                    beyond.append(f"{entry} bh_kv={bh} len={n}: a / b = {med['a', n] / b:.3f} (allowed {100 * allowed:.1f} %)")
            for n0 in (8192, 8193):
                r = med["a", n0 + 24576] / med["a", n0]
                by_len.append(f"{entry} bh_kv={bh}: a({n0 + 24576}) / a({n0}) = {r:.3f}" + (" (beyond b's spread)" if abs(r - 1.0) > spread_b else ""))
            del arms
        del c
        torch.cuda.empty_cache()
    say()
    say("a / b beyond the allowed terms: " + ("; ".join(beyond) or "none"))
    say()
    say("does a depend on len?  " + "; ".join(by_len))

    # profiles/kv_window_fp8.txt: the run as printed; docs/kv_window_fp8.md: the same tables between the two markers, the prose around them is kept
    out_txt = os.path.join(a.out_dir or os.path.join(ROOT, "profiles"), "kv_window_fp8.txt")
    out_md = os.path.join(a.out_dir or os.path.join(ROOT, "docs"), "kv_window_fp8.md")
    os.makedirs(os.path.dirname(out_txt), exist_ok=True)
    body = "\n".join(lines) + "\n"
    with open(out_txt, "w") as f:
        f.write(body)
    begin, end = "<!-- measured:begin -->\n", "<!-- measured:end -->\n"
    doc = os.path.join(ROOT, "docs", "kv_window_fp8.md")
    text = open(doc).read() if os.path.exists(doc) else f"# Sliding-window attention over the fp8 KV caches: measurements\n\n{begin}{end}"
    head, rest = text.split(begin)
    with open(out_md, "w") as f:
        f.write(head + begin + body + end + rest.split(end)[1])


if __name__ == "__main__":
    main()
