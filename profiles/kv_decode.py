"""Measurement of the KV-cache decode kernel (include/flashattn_amd_kv.h): writes profiles/kv_decode.txt and docs/kv_decode.md.

    python profiles/kv_decode.py --build-variants        # CPU: the measurement builds (plan constants, one-term P) -> profiles/kv_variants/
    python profiles/kv_decode.py [--out-dir DIR]         # GPU: one run, its own time limit is the caller's (about four minutes)
    python profiles/kv_decode.py --trace-shape 64,8192   # GPU, for `rocprofv3 --kernel-trace --stats -- python ...`: arms a and b only

Shapes: d = 128, nq = 1, bf16 output, bh_kv in {8, 64, 512}, nk in {2048, 8192, 32768}, group 8 (and group 1 at equal bh_kv).
Arms per shape, device events around >= 200 warmed launches on one stream, rotating over enough distinct K/V buffers that the footprint
exceeds the 256 MB Infinity Cache, alternated and repeated three times (medians are reported, the spread of b is its max - min):
  a  fa_kv_forward                      b  fa_kv_stream_read on the same buffers (the floor)
  c  the only route before the extension: Q zero-padded to nk rows through the square causal fa.forward, last row kept (where it fits)
  d  torch SDPA with expanded K/V (information only)
Then the sweep over the two plan constants of csrc/fa_kv.h and the A/B of the second P.V product (measurement builds, never shipped).
"""
from __future__ import annotations

import argparse
import ctypes
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT_DIR = os.path.join(ROOT, "profiles", "kv_variants")
TARGETS, MIN_SHARES = (128, 256, 512, 1024), (128, 256, 512, 1024)
D, GROUP = 128, 8
SHAPES = [(bh, nk) for bh in (8, 64, 512) for nk in (2048, 8192, 32768)]
LAUNCHES, REPEATS = 200, 3
ROTATE_BYTES = 1 << 30            # K + V over all rotated buffers: four times the Infinity Cache
SQUARE_FLOP_LIMIT = 4e13          # arm c beyond this (>~ 50 ms per call) is skipped: its n^2 work is the point, not worth the GPU time


def variants():
    return [(f"t{t}_m{m}", [f"FA_KV_TARGET_WGS={t}", f"FA_KV_MIN_SHARE={m}"]) for t in TARGETS for m in MIN_SHARES] + [("p1", ["FA_KV_P_TERMS=1"])]


def build_variants():
    spec = importlib.util.spec_from_file_location("fa_build", os.path.join(ROOT, "flashattention.c_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tag, defines in variants():
        print(mod.build_kv_variant(tag, defines, VARIANT_DIR))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--out-dir", default=None, help="write kv_decode.txt / kv_decode.md here instead of profiles/ and docs/")
    ap.add_argument("--trace-shape", default=None, help="bh_kv,nk: run arms a and b 50 times each and exit (for rocprofv3)")
    ap.add_argument("--quick", action="store_true", help="rehearsal: 2 shapes, 20 launches")
    a = ap.parse_args()
    if a.build_variants:
        return build_variants()

    import torch
    import torch.nn.functional as F
    import flashattention_c_amd as fa
    from flashattention_c_amd import _cabi_kv
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    BF16 = _cabi_kv.FA_DTYPE_BF16
    LIB = _cabi_kv.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    class Case:
        """the buffers of one shape: nbuf rotated K/V caches, q / o / workspace for group 8 and group 1"""

        def __init__(self, bh, nk):
            self.bh, self.nk = bh, nk
            self.kv_bytes = 2 * bh * nk * D * 2
            self.nbuf = max(1, -(-ROTATE_BYTES // self.kv_bytes))
            self.k = torch.empty(self.nbuf, bh, nk, D, dtype=torch.bfloat16, device=dev).normal_()
            self.v = torch.empty(self.nbuf, bh, nk, D, dtype=torch.bfloat16, device=dev).normal_()
            self.q = {g: torch.randn(bh * g, 1, D, device=dev).to(torch.bfloat16) for g in (GROUP, 1)}
            self.o = {g: torch.empty(bh * g, 1, D, dtype=torch.bfloat16, device=dev) for g in (GROUP, 1)}
            self.sink = torch.zeros(1024, dtype=torch.int32, device=dev)
            self.ws = {}

        def forward(self, L, g, i):
            key = (id(L), g)
            if key not in self.ws:
                need = int(L.fa_kv_workspace_bytes(self.bh, g, 1, self.nk, D, 0, BF16))
                self.ws[key] = torch.empty(max(need, 256), dtype=torch.uint8, device=dev), need
            ws, need = self.ws[key]
            j = i % self.nbuf
            rc = L.fa_kv_forward(self.q[g].data_ptr(), self.k[j].data_ptr(), self.v[j].data_ptr(), self.o[g].data_ptr(), None, self.bh, g, 1, self.nk, self.nk,
                                 None, D, 0.088, 0, BF16, ws.data_ptr() if need else None, need, stream())
            assert rc == 0, L.fa_kv_last_error()

        def stream_read(self, i):
            j = i % self.nbuf
            assert LIB.fa_kv_stream_read(self.k[j].data_ptr(), self.v[j].data_ptr(), self.bh, self.nk, self.nk, D, self.sink.data_ptr(), stream()) == 0

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
        timed(lambda i: c.forward(LIB, GROUP, i), 50)
        timed(c.stream_read, 50)
        return

    shapes = SHAPES[:2] if a.quick else SHAPES
    launches = 20 if a.quick else LAUNCHES
    free, total = torch.cuda.mem_get_info()
    say(f"# {LIB.fa_kv_version().decode()}; {torch.cuda.get_device_name(0)}; {launches} launches per timing, {REPEATS} repeats (median; spread = max - min)")
    say()
    say("## arms")
    say("| bh_kv | nk | K+V MB | buffers | S | a: fa_kv_forward us | a GB/s | b: stream read us | b spread us | a/b | group 8 / group 1 | c: padded square us | c/a | d: SDPA us |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    explain = []
    for bh, nk in shapes:
        kv = 2 * bh * nk * D * 2
        if 2.5 * max(kv, ROTATE_BYTES) > free:
            say(f"| {bh} | {nk} | {kv / 2**20:.0f} | skipped: K + V exceed the free memory |")
            continue
        c = Case(bh, nk)
        S = LIB.fa_kv_splits_for(bh, GROUP, 1, nk, D, 0, BF16)
        arms = {"a": lambda i: c.forward(LIB, GROUP, i), "a1": lambda i: c.forward(LIB, 1, i), "b": c.stream_read}
        n_c = 0
        flop = 2.0 * nk * nk * D * bh * GROUP          # causal square: half of 4 n^2 d per slab
        if flop <= SQUARE_FLOP_LIMIT and 4 * bh * GROUP * nk * D * 2 < free // 2:
            qp = torch.zeros(bh * GROUP, nk, D, dtype=torch.bfloat16, device=dev)
            qp[:, -1:] = c.q[GROUP]
            ke, ve = (t[0].repeat_interleave(GROUP, dim=0) for t in (c.k, c.v))   # the square entry has no groups: K/V once per query head
            op = torch.empty_like(qp)
            arms["c"] = lambda i: fa.forward(qp, ke, ve, True, scale=0.088, out=op)
            n_c = max(3, min(20, int(2e12 / flop) + 1))
        try:
            if kv * GROUP > 8e9:
                raise MemoryError("expanded K/V too large")
            qs = c.q[GROUP].view(bh, GROUP, 1, D)
            F.scaled_dot_product_attention(qs, c.k[0].unsqueeze(1).expand(bh, GROUP, nk, D), c.v[0].unsqueeze(1).expand(bh, GROUP, nk, D), scale=0.088)
            arms["d"] = lambda i: F.scaled_dot_product_attention(qs, c.k[i % c.nbuf].unsqueeze(1).expand(bh, GROUP, nk, D),
                                                                 c.v[i % c.nbuf].unsqueeze(1).expand(bh, GROUP, nk, D), scale=0.088)
        except Exception as e:   # information only
            say(f"(SDPA unavailable at bh_kv={bh} nk={nk}: {type(e).__name__})")
        t = {k: [] for k in arms}
        for _ in range(REPEATS):
            for k, fn in arms.items():
                t[k].append(timed(fn, n_c if k == "c" else (max(10, launches // 10) if k == "d" else launches)))
        med = {k: statistics.median(x) for k, x in t.items()}
        spread_b = max(t["b"]) - min(t["b"])
        say(f"| {bh} | {nk} | {kv / 2**20:.0f} | {c.nbuf} | {S} | {med['a']:.1f} | {kv / med['a'] / 1e3:.0f} | {med['b']:.1f} | {spread_b:.1f} | {med['a'] / med['b']:.2f} | "
            f"{med['a'] / med['a1']:.2f} | {med.get('c', float('nan')):.1f} | {med.get('c', float('nan')) / med['a']:.0f} | {med.get('d', float('nan')):.1f} |")
        if "c" in med:
            assert med["a"] <= med["c"], f"fa_kv_forward slower than the padded square route at bh_kv={bh} nk={nk}"
        if kv * c.nbuf >= 1e9 and med["a"] - med["b"] > 2 * spread_b:
            explain.append((bh, nk, med["a"] / med["b"]))
        del c, arms
        torch.cuda.empty_cache()
    say()
    say("a/b beyond the floor's own spread (needs the explanation from the kernel trace): " + (", ".join(f"bh_kv={b} nk={n}: {r:.2f}" for b, n, r in explain) or "none"))

    def compare(tags, title):
        say()
        say(f"## {title}")
        say("us per launch of fa_kv_forward, group 8 (median of 3, arms alternated); last column: geometric mean over the shapes of time / time of the shipped build")
        libs = {"shipped": LIB}
        for tag in tags:
            p = os.path.join(VARIANT_DIR, f"libflashattn_amd_kv_{tag}.so")
            if os.path.exists(p):
                libs[tag] = _cabi_kv.bind(p)
        say("| build | " + " | ".join(f"{bh} x {nk}" for bh, nk in shapes) + " | geomean |")
        say("|---|" + "---|" * (len(shapes) + 1))
        res = {k: [] for k in libs}
        splits = {k: [] for k in libs}
        for bh, nk in shapes:
            if 2.5 * max(2 * bh * nk * D * 2, ROTATE_BYTES) > free:
                continue
            c = Case(bh, nk)
            t = {k: [] for k in libs}
            for _ in range(REPEATS):
                for k, L in libs.items():
                    t[k].append(timed(lambda i: c.forward(L, GROUP, i), launches))
            for k, L in libs.items():
                res[k].append(statistics.median(t[k]))
                splits[k].append(L.fa_kv_splits_for(bh, GROUP, 1, nk, D, 0, BF16))
            del c
            torch.cuda.empty_cache()
        for k in libs:
            gm = statistics.geometric_mean([x / y for x, y in zip(res[k], res["shipped"])])
            say(f"| {k} | " + " | ".join(f"{x:.1f} (S={s})" for x, s in zip(res[k], splits[k])) + f" | {gm:.3f} |")

    compare([tag for tag, _ in variants() if tag != "p1"], "plan constants: t<target workgroups>_m<minimum keys per share>")
    compare(["p1"], "is the second P.V product free?  p1 = P as ONE bf16 term (wrong to 2^-9; a measurement build only)")

    # profiles/kv_decode.txt: the run as printed; docs/kv_decode.md: the same tables between the two markers, the prose around them is kept
    out_txt = os.path.join(a.out_dir or os.path.join(ROOT, "profiles"), "kv_decode.txt")
    out_md = os.path.join(a.out_dir or os.path.join(ROOT, "docs"), "kv_decode.md")
    os.makedirs(os.path.dirname(out_txt), exist_ok=True)
    body = "\n".join(lines) + "\n"
    with open(out_txt, "w") as f:
        f.write(body)
    begin, end = "<!-- measured:begin -->\n", "<!-- measured:end -->\n"
    doc = os.path.join(ROOT, "docs", "kv_decode.md")
    text = open(doc).read() if os.path.exists(doc) else f"# KV-cache decode: measurements\n\n{begin}{end}"
    head, rest = text.split(begin)
    with open(out_md, "w") as f:
        f.write(head + begin + body + end + rest.split(end)[1])


if __name__ == "__main__":
    main()
