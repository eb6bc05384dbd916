"""Measurement of KV-cache attention over an fp8 cache (include/flashattn_amd_kv8.h): writes profiles/kv_fp8.txt and docs/kv_fp8.md.

    python profiles/kv_fp8.py [--out-dir DIR]          # GPU: one run (about half a minute; the largest shape holds 21 GB while it is checked)

Shapes: d = 128, nq = 1, group 8, bf16 output, bh_kv x nk over {8, 64, 512} x {2048, 8192, 32768} (the row counts of docs/kv_decode.md).
The timing method is profiles/kv_decode.py's: device events around 200 warmed launches on one stream, rotating over enough distinct K/V buffers
that the fp8 footprint is 1 GB (four times the 256 MB Infinity Cache; the bf16 twin's is twice that), arms alternated, three repeats, medians;
the spread of an arm is (max - min) / median.
Arms per shape:
  a  fa_kv_forward on a bf16 cache (bh_kv, nk, d): unchanged code, the baseline.  The cache is the fp8 one dequantised: arm b's twin
  b  fa_kv8_forward on the fp8 cache of the same rows: half the K/V bytes
  c  the floor for half the bytes: fa_kv_stream_read on the fp8 buffers with d = 64 (a 128-byte row is 64 bf16 columns: exactly those bytes)
  p  fa_kv8_paged_forward on the memory of arm b seen as a pool (bh_kv * nk / page, page, d), pages of 16 and 256 rows, with an identity table
     and a shuffled one (one random permutation of all pages of the buffer)
Every fp8 arm is checked bit for bit against its bf16 twin (fa_kv_forward on the dequantised cache its table describes; k_scale = v_scale = 1)
before it is timed.  The script asserts one thing about the times: at 512 x 8192 and 512 x 32768, where arm a runs at the rate of a streaming
read of its bytes, arm b is not slower than arm a.
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
SHAPES = [(bh, nk) for bh in (8, 64, 512) for nk in (2048, 8192, 32768)]
MUST_NOT_LOSE = [(512, 8192), (512, 32768)]
PAGES = (16, 256)
LAUNCHES, REPEATS = 200, 3
ROTATE_BYTES = 1 << 30            # fp8 K + V over all rotated buffers: four times the Infinity Cache


def e4m3_table():
    """the 256 values of OCP e4m3fn (tests/kv8_reference.py has the same table; this script stands alone)"""
    out = []
    for c in range(256):
        s, e, m = (-1.0 if c & 0x80 else 1.0), (c >> 3) & 0xF, c & 7
        out.append(float("nan") if (e, m) == (15, 7) else s * (m / 8.0) * 2.0 ** -6 if e == 0 else s * (1 + m / 8.0) * 2.0 ** (e - 7))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None, help="write kv_fp8.txt / kv_fp8.md here instead of profiles/ and docs/")
    ap.add_argument("--quick", action="store_true", help="rehearsal: the first shape, 20 launches")
    a = ap.parse_args()

    import torch
    from flashattention_c_amd import _cabi_kv, _cabi_kv8
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    BF16 = _cabi_kv.FA_DTYPE_BF16
    KV, K8 = _cabi_kv.lib(), _cabi_kv8.lib()
    lut = torch.tensor(e4m3_table(), dtype=torch.float32).to(torch.bfloat16).to(dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dequant_into(dst, src):
        """bf16 dst <- the values of the e4m3 bytes src, by table (exact), in pieces"""
        d, s = dst.view(-1), src.view(-1)
        for i in range(0, s.numel(), 1 << 26):
            d[i:i + (1 << 26)] = lut[s[i:i + (1 << 26)].long()]

    class Case:
        """the buffers of one shape: nbuf rotated fp8 K/V caches and their bf16 twins, q / o / workspace, and the block tables"""

        def __init__(self, bh, nk):
            self.bh, self.nk = bh, nk
            self.kv8_bytes = 2 * bh * nk * D
            self.nbuf = max(1, -(-ROTATE_BYTES // self.kv8_bytes))
            # random bytes with the top exponent bit cleared: every sign and mantissa, |value| < 2, no NaN code
            self.k8, self.v8 = (torch.randint(0, 256, (self.nbuf, bh, nk, D), dtype=torch.uint8, device=dev) & 0xBF for _ in range(2))
            self.k, self.v = (torch.empty(self.nbuf, bh, nk, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
            dequant_into(self.k, self.k8)
            dequant_into(self.v, self.v8)
            self.q = torch.randn(bh * GROUP, 1, D, device=dev).to(torch.bfloat16)
            self.o = torch.empty(bh * GROUP, 1, D, dtype=torch.bfloat16, device=dev)
            self.sink = torch.zeros(1024, dtype=torch.int32, device=dev)
            need = int(KV.fa_kv_workspace_bytes(bh, GROUP, 1, nk, D, 0, BF16))
            assert need == int(K8.fa_kv8_workspace_bytes(bh, GROUP, 1, nk, D, 0, BF16))
            self.ws, self.need = torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need
            self.tables = {}
            gen = torch.Generator().manual_seed(bh * 131 + nk)
            for page in PAGES:
                n = bh * nk // page
                ident = torch.arange(n, dtype=torch.int32)
                self.tables[page, "identity"] = ident.view(bh, nk // page).to(dev)
                self.tables[page, "shuffled"] = ident[torch.randperm(n, generator=gen)].view(bh, nk // page).contiguous().to(dev)
            # the cache descriptors, built once: the timed loop of a paged arm does the host work of the others, one foreign call per launch
            self.caches = {(page, kind, j): _cabi_kv8.FaPagedCache(self.k8[j].data_ptr(), self.v8[j].data_ptr(), bh * nk // page, page, page * D, D, 0,
                                                                   t.data_ptr(), nk // page, None)
                           for (page, kind), t in self.tables.items() for j in range(self.nbuf)}

        def wsp(self):
            return (self.ws.data_ptr() if self.need else None), self.need

        def bf16(self, i, k=None, v=None):
            j = i % self.nbuf
            k, v = (self.k[j], self.v[j]) if k is None else (k, v)
            rc = KV.fa_kv_forward(self.q.data_ptr(), k.data_ptr(), v.data_ptr(), self.o.data_ptr(), None, self.bh, GROUP, 1, self.nk, self.nk,
                                  None, D, 0.088, 0, BF16, *self.wsp(), stream())
            assert rc == 0, KV.fa_kv_last_error()

        def fp8(self, i):
            j = i % self.nbuf
            rc = K8.fa_kv8_forward(self.q.data_ptr(), self.k8[j].data_ptr(), self.v8[j].data_ptr(), self.o.data_ptr(), None, self.bh, GROUP, 1, self.nk, self.nk,
                                   None, D, 0.088, 1.0, 1.0, 0, BF16, *self.wsp(), stream())
            assert rc == 0, K8.fa_kv8_last_error()

        def paged(self, page, kind, i):
            rc = K8.fa_kv8_paged_forward(self.q.data_ptr(), ctypes.byref(self.caches[page, kind, i % self.nbuf]), self.o.data_ptr(), None, self.bh, 1, GROUP, 1,
                                         self.nk, D, 0.088, 1.0, 1.0, 0, BF16, *self.wsp(), stream())
            assert rc == 0, K8.fa_kv8_last_error()

        def floor(self, i):
            j = i % self.nbuf   # the fp8 bytes read as rows of 64 bf16 columns
            assert KV.fa_kv_stream_read(self.k8[j].data_ptr(), self.v8[j].data_ptr(), self.bh, self.nk, self.nk, D // 2, self.sink.data_ptr(), stream()) == 0

        def check(self):
            """every fp8 arm gives, to the bit, what fa_kv_forward gives on the bf16 twin of the cache it reads: buffer 0 itself for the contiguous
            arm and the identity tables, a gathered copy under a shuffled table"""
            def result(fn):
                self.o.zero_()
                fn()
                return self.o.clone()
            want = result(lambda: self.bf16(0))
            assert torch.equal(result(lambda: self.fp8(0)).view(torch.int16), want.view(torch.int16)), "fa_kv8_forward differs from its bf16 twin"
            for (page, kind), t in self.tables.items():
                kc, vc = (x[0].view(-1, page, D)[t.long()].reshape(self.bh, self.nk, D) for x in (self.k, self.v))
                want = result(lambda: self.bf16(0, kc, vc))
                assert torch.equal(result(lambda: self.paged(page, kind, 0)).view(torch.int16), want.view(torch.int16)), (page, kind)
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

    shapes = SHAPES[:1] if a.quick else SHAPES
    launches = 20 if a.quick else LAUNCHES
    free, _ = torch.cuda.mem_get_info()
    say(f"# {K8.fa_kv8_version().decode()}; {torch.cuda.get_device_name(0)}; {launches} launches per timing, {REPEATS} repeats (median; spread = (max - min) / median)")
    say()
    say("us per launch.  d = 128, nq = 1, group 8, bf16 output, k_scale = v_scale = 1.  a: fa_kv_forward on the bf16 twin; b: fa_kv8_forward; c: fa_kv_stream_read")
    say("over the fp8 bytes (the floor for half the bytes); p<page>: fa_kv8_paged_forward over arm b's memory, p / b in brackets.  Every fp8 arm was checked,")
    say("before it was timed, to give bit for bit what fa_kv_forward gives on the dequantised cache.")
    say()
    heads = [f"p{page} {kind}" for page in PAGES for kind in ("identity", "shuffled")]
    say("| bh_kv x nk | fp8 K+V MB | buffers | S | a: bf16 | a GB/s | a spread | b: fp8 | b GB/s | b spread | b / a | c: floor | c spread | b / c | " + " | ".join(heads) + " |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|" + "---|" * len(heads))
    beyond, lost = [], []
    for bh, nk in shapes:
        kv8 = 2 * bh * nk * D
        if 3.5 * max(kv8, ROTATE_BYTES) > free:   # the fp8 buffers, twins of twice their size, and the gathered copies of the check
            say(f"| {bh} x {nk} | {kv8 / 2**20:.0f} | skipped: the buffers exceed the free memory |")
            continue
        c = Case(bh, nk)
        c.check()
        S = K8.fa_kv8_splits_for(bh, GROUP, 1, nk, D, 0, BF16)
        assert S == KV.fa_kv_splits_for(bh, GROUP, 1, nk, D, 0, BF16)
        arms = {"a": c.bf16, "b": c.fp8, "c": c.floor}
        for page in PAGES:
            for kind in ("identity", "shuffled"):
                arms[f"p{page} {kind}"] = lambda i, page=page, kind=kind: c.paged(page, kind, i)
        t = {k: [] for k in arms}
        for _ in range(REPEATS):
            for k, fn in arms.items():
                t[k].append(timed(fn, launches))
        med = {k: statistics.median(x) for k, x in t.items()}
        spread = {k: (max(x) - min(x)) / statistics.median(x) for k, x in t.items()}
        say(f"| {bh} x {nk} | {kv8 / 2**20:.0f} | {c.nbuf} | {S} | {med['a']:.1f} | {2 * kv8 / med['a'] / 1e3:.0f} | {100 * spread['a']:.1f} % | "
            f"{med['b']:.1f} | {kv8 / med['b'] / 1e3:.0f} | {100 * spread['b']:.1f} % | {med['b'] / med['a']:.3f} | "
            f"{med['c']:.1f} | {100 * spread['c']:.1f} % | {med['b'] / med['c']:.3f} | "
            + " | ".join(f"{med[h]:.1f} ({med[h] / med['b']:.3f})" for h in heads) + " |")
        if med["b"] / med["c"] - 1.0 > spread["c"]:
            beyond.append(f"{bh} x {nk}: {med['b'] / med['c']:.3f} (c's spread {100 * spread['c']:.1f} %, b's own {100 * spread['b']:.1f} %)")
        if (bh, nk) in MUST_NOT_LOSE and med["b"] > med["a"]:
            lost.append(f"{bh} x {nk}: b {med['b']:.1f} us, a {med['a']:.1f} us")
        del c, arms
        torch.cuda.empty_cache()
    say()
    say("b / c beyond the spread of arm c's own repeats: " + ("; ".join(beyond) or "none"))

    # profiles/kv_fp8.txt: the run as printed; docs/kv_fp8.md: the same tables between the two markers, the prose around them is kept
    out_txt = os.path.join(a.out_dir or os.path.join(ROOT, "profiles"), "kv_fp8.txt")
    out_md = os.path.join(a.out_dir or os.path.join(ROOT, "docs"), "kv_fp8.md")
    os.makedirs(os.path.dirname(out_txt), exist_ok=True)
    body = "\n".join(lines) + "\n"
    with open(out_txt, "w") as f:
        f.write(body)
    begin, end = "<!-- measured:begin -->\n", "<!-- measured:end -->\n"
    doc = os.path.join(ROOT, "docs", "kv_fp8.md")
    text = open(doc).read() if os.path.exists(doc) else f"# KV-cache attention over an fp8 cache: measurements\n\n{begin}{end}"
    head, rest = text.split(begin)
    with open(out_md, "w") as f:
        f.write(head + begin + body + end + rest.split(end)[1])
    assert not lost, "half the bytes and not faster -- " + "; ".join(lost)


if __name__ == "__main__":
    main()
