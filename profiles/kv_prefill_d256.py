"""Measurements behind docs/kv_prefill_d256.md: the chunked-prefill kernel at head dim 256 (libflashattn_amd_kvp256.so) against the decode kernel
of libflashattn_amd_kv256.so on the same tensors, by the method of profiles/kv_prefill.py -- warmed launches on one stream, device events, arms
alternated, three repeats, median with min .. max.

  a  fa.prefill_kv (fa.prefill_paged on the paged row)
  b  fa.forward_kv (fa.forward_paged) on the same tensors, with its workspace: the decode kernel, the only route before this library

d = 256, bf16 output, scale 0.0625.  FLOP are counted as 4 d per visible (row, key) pair; wgs is a's grid, bh_kv * ceil(group * nq / 128).

    python profiles/kv_prefill_d256.py [--out FILE] [--quick]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, SCALE, REPEATS, ROW_TILE = 256, 0.0625, 3, 128
# (label, bh_kv, group, nq, nk, causal, page): page = 0 for a contiguous cache
SHAPES = [
    ("chunk", 8, 4, 2048, 2048, True, 0), ("chunk", 8, 4, 2048, 8192, True, 0), ("chunk", 8, 4, 2048, 32768, True, 0),
    ("sweep", 8, 4, 16, 8192, True, 0), ("sweep", 8, 4, 64, 8192, True, 0), ("sweep", 8, 4, 256, 8192, True, 0), ("sweep", 8, 4, 1024, 8192, True, 0),
    ("paged 16", 8, 4, 2048, 8192, True, 16),
]


def visible_pairs(bh_kv, group, nq, nk, causal):
    rows = bh_kv * group
    if not causal:
        return rows * nq * nk
    return rows * sum(max(0, min(nk, nk - nq + i + 1)) for i in range(nq))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="rehearsal: the shapes below 10^11 FLOP, few launches")
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

    def fmt(x, flop):
        return f"{x[0]:.1f} ({x[1]:.1f} .. {x[2]:.1f}) / {flop / x[0] / 1e6:.0f}"

    say("| shape | bh_kv | group | nq | nk | causal | wgs | a: prefill us / TFLOP/s | b: decode kernel us / TFLOP/s | a/b | beyond both spreads |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for label, bh_kv, group, nq, nk, causal, page in SHAPES:
        flop = 4 * D * visible_pairs(bh_kv, group, nq, nk, causal)
        if a.quick and flop > 1e11:
            continue
        q = torch.randn(bh_kv * group, nq, D, device=dev).to(torch.bfloat16)
        k, v = (torch.randn(bh_kv, nk, D, device=dev).to(torch.bfloat16) for _ in range(2))
        o = torch.empty_like(q)
        if page:   # the same cache as pages of `page` rows of one head under a shuffled table
            table = torch.randperm(bh_kv * (nk // page), device=dev).to(torch.int32).reshape(bh_kv, nk // page)
            kp, vp = (torch.empty(bh_kv * (nk // page), page, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
            kp[table.flatten().long()] = k.view(-1, page, D)
            vp[table.flatten().long()] = v.view(-1, page, D)
            ws = torch.empty(max(fa.workspace_bytes_paged(bh_kv, 1, group, nq, nk, D, causal), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: fa.prefill_paged(q, kp, vp, table, causal, scale=SCALE, out=o),
                    "b": lambda: fa.forward_paged(q, kp, vp, table, causal, scale=SCALE, out=o, workspace=ws)}
        else:
            ws = torch.empty(max(fa.workspace_bytes_kv(bh_kv, group, nq, nk, D, causal), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: fa.prefill_kv(q, k, v, causal, scale=SCALE, out=o),
                    "b": lambda: fa.forward_kv(q, k, v, causal, scale=SCALE, out=o, workspace=ws)}
        r = measure(arms)
        apart = r["a"][2] < r["b"][1] or r["b"][2] < r["a"][1]
        say(f"| {label} | {bh_kv} | {group} | {nq} | {nk} | {int(causal)} | {bh_kv * -(-group * nq // ROW_TILE)} | {fmt(r['a'], flop)} | {fmt(r['b'], flop)} | "
            f"{r['a'][0] / r['b'][0]:.3f} | {'yes' if apart else 'no'} |")
        del q, k, v, o

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
