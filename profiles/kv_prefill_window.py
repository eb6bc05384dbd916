"""Measurements behind docs/kv_prefill_window.md: chunked prefill under a sliding window (libflashattn_amd_kvpw.so) against the decode kernels
under the same window and against the unwindowed prefill kernel over as many keys as a tile walks, by the method of profiles/kv_prefill_d256.py
-- warmed launches on one stream, device events, arms alternated in one process, three repeats, median with min .. max.

  a  fa.prefill_kv / prefill_kv_fp8 (prefill_paged* on the paged rows) with window_left
  b  fa.forward_kv / forward_kv_fp8 (forward_paged*) with the same window_left and its workspace: the only correct route before this library
  c  a without window_left on the first window_left + 1 + nq keys of the same tensors: the same walk without the window logic -- ANOTHER
     function (full causal attention over those keys), timed for its cost only

bh_kv = 8, group 4, nq = 2048, causal, window_left = 4095, bf16 output, scale 0.0625.  wgs is a's grid, bh_kv * ceil(group * nq / row tile).

    python profiles/kv_prefill_window.py [--out FILE] [--quick]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE, REPEATS, BH_KV, GROUP, NQ, WINDOW = 0.0625, 3, 8, 4, 2048, 4095
KS, VS = 0.013, 0.011
# (label, d, fp8, nk, page): page = 0 for a contiguous cache
SHAPES = [(f"{'fp8' if fp8 else 'bf16'} d={d}" + (f" paged {page}" if page else ""), d, fp8, nk, page)
          for d, fp8 in ((128, False), (128, True), (256, False)) for nk, page in ((8192, 0), (32768, 0), (8192, 16))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="rehearsal: few launches")
    a = ap.parse_args()

    import torch
    import flashattention_c_amd as fa
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, launches):
        for _ in range(max(2, launches // 10)):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    def measure(arms):
        """arms alternated within a repeat; launches from a pilot, about 40 ms per timing; median and (min, max) of the repeats, microseconds"""
        n = {k: 3 if a.quick else int(min(200, max(3, 40e3 // timed(fn, 2)))) for k, fn in arms.items()}
        t = {k: [] for k in arms}
        for _ in range(REPEATS):
            for k, fn in arms.items():
                t[k].append(timed(fn, n[k]))
        return {k: (statistics.median(x), min(x), max(x)) for k, x in t.items()}

    def fmt(x):
        return f"{x[0]:.1f} ({x[1]:.1f} .. {x[2]:.1f})"

    def apart(x, y):
        return "yes" if x[2] < y[1] or y[2] < x[1] else "no"

    say("| cache | nk | wgs | a: windowed prefill us | b: windowed decode kernel us | c: unwindowed prefill, 6144 keys us | a/b | beyond both spreads | a/c |")
    say("|---|---|---|---|---|---|---|---|---|")
    results = {}
    for label, d, fp8, nk, page in SHAPES:
        q = torch.randn(BH_KV * GROUP, NQ, d, device=dev).to(torch.bfloat16)
        k, v = (torch.randn(BH_KV, nk, d, device=dev) for _ in range(2))
        if fp8:
            k, v = (k / KS).clamp(-448, 448).to(torch.float8_e4m3fn), (v / VS).clamp(-448, 448).to(torch.float8_e4m3fn)
            kw = dict(k_scale=KS, v_scale=VS)
        else:
            k, v, kw = k.to(torch.bfloat16), v.to(torch.bfloat16), {}
        o = torch.empty_like(q)
        kw.update(scale=SCALE, out=o)
        sfx = "_fp8" if fp8 else ""
        nc = WINDOW + 1 + NQ   # the keys arm c walks
        if page:   # the same cache as pages of `page` rows of one head under a shuffled table
            prefill, decode = getattr(fa, "prefill_paged" + sfx), getattr(fa, "forward_paged" + sfx)
            table = torch.randperm(BH_KV * (nk // page), device=dev).to(torch.int32).reshape(BH_KV, nk // page)
            kp, vp = (torch.empty(BH_KV * (nk // page), page, d, dtype=k.dtype, device=dev).view(torch.uint8) for _ in range(2))
            kp[table.flatten().long()] = k.view(torch.uint8).view(BH_KV * (nk // page), page, -1)
            vp[table.flatten().long()] = v.view(torch.uint8).view(BH_KV * (nk // page), page, -1)
            kp, vp = kp.view(k.dtype), vp.view(k.dtype)
            ws = torch.empty(max(fa.workspace_bytes_paged(BH_KV, 1, GROUP, NQ, nk, d, True, window_left=WINDOW), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: prefill(q, kp, vp, table, True, window_left=WINDOW, **kw),
                    "b": lambda: decode(q, kp, vp, table, True, window_left=WINDOW, workspace=ws, **kw),
                    "c": lambda: prefill(q, kp, vp, table, True, kv_len=nc, **kw)}
        else:
            prefill, decode = getattr(fa, "prefill_kv" + sfx), getattr(fa, "forward_kv" + sfx)
            ws = torch.empty(max(fa.workspace_bytes_kv(BH_KV, GROUP, NQ, nk, d, True, window_left=WINDOW), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: prefill(q, k, v, True, window_left=WINDOW, **kw),
                    "b": lambda: decode(q, k, v, True, window_left=WINDOW, workspace=ws, **kw),
                    "c": lambda: prefill(q, k, v, True, kv_len=nc, **kw)}
        r = results[label, nk] = measure(arms)
        say(f"| {label} | {nk} | {BH_KV * -(-GROUP * NQ // (128 if d == 256 else 256))} | {fmt(r['a'])} | {fmt(r['b'])} | {fmt(r['c'])} | "
            f"{r['a'][0] / r['b'][0]:.3f} | {apart(r['a'], r['b'])} | {r['a'][0] / r['c'][0]:.3f} |")
        del q, k, v, o
    say()
    say("| cache | a at nk = 32768 / a at nk = 8192 | equal within spread |")
    say("|---|---|---|")
    for label, d, fp8, nk, page in SHAPES:
        if nk == 8192 and not page:
            lo, hi = results[label, 8192]["a"], results[label, 32768]["a"]
            say(f"| {label} | {hi[0] / lo[0]:.3f} | {'yes' if apart(lo, hi) == 'no' else 'no'} |")

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
