"""Measurements behind docs/kv_prefill_fp8.md: the fp8 chunked-prefill kernel (libflashattn_amd_kvp8.so) against the fp8 decode kernel on the
same tensors and against the bf16 prefill kernel on the dequantised cache, by the method of profiles/kv_prefill.py -- warmed launches on one
stream, device events, arms alternated in one process, three repeats, median with min .. max.

  a  fa.prefill_kv_fp8 (fa.prefill_paged_fp8 on the paged rows)
  b  fa.forward_kv_fp8 (fa.forward_paged_fp8) on the same tensors, with its workspace: the decode kernel, the only route before this library
  c  fa.prefill_kv (fa.prefill_paged) on the cache dequantised to bf16: the same loop without the conversion

d = 128, bf16 output, scale 0.088, k_scale 0.013, v_scale 0.011.  Before a shape is timed, the outputs of a and b must agree to the bf16-output
bar of the tests (2.5e-2).  FLOP are counted as 4 d per visible (row, key) pair.

    python profiles/kv_prefill_fp8.py [--out FILE] [--quick]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.kv_prefill import visible_pairs  # noqa: E402

D, SCALE, KS, VS, REPEATS, TOL_BF16 = 128, 0.088, 0.013, 0.011, 3, 2.5e-2
# (label, bh_kv, group, nq, nk, causal, page): page = 0 for a contiguous cache
SHAPES = [(lab, 8, 4, 2048, nk, True, page) for lab, page in (("chunk", 0), ("paged 16", 16)) for nk in (2048, 8192, 32768)] + \
         [("sweep", 8, 4, nq, 8192, True, 0) for nq in (16, 64, 256, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="rehearsal: the shapes below 10^11 FLOP, few launches")
    a = ap.parse_args()

    import torch
    import flashattention_c_amd as fa
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    F8 = torch.float8_e4m3fn
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

    def beyond(x, y):
        return "yes" if x[2] < y[1] or y[2] < x[1] else "no"

    def fp8(shape, scale):
        """N(0, 1) quantised at `scale` on the CPU (no fp8 arithmetic of torch's runs on the GPU); the bytes and their exact bf16 twin on the device"""
        t8 = (torch.randn(*shape) / scale).clamp(-448.0, 448.0).to(F8)
        return t8.view(torch.uint8).to(dev).view(F8), t8.to(torch.bfloat16).to(dev)

    say("| shape | bh_kv | group | nq | nk | workgroups | a: fp8 prefill us / TFLOP/s | b: fp8 decode kernel us / TFLOP/s | c: bf16 prefill us / TFLOP/s | a/b | a vs b beyond the spread | a/c | a vs c beyond the spread |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for label, bh_kv, group, nq, nk, causal, page in SHAPES:
        flop = 4 * D * visible_pairs(bh_kv, group, nq, nk, causal)
        if a.quick and flop > 1e11:
            continue
        q = torch.randn(bh_kv * group, nq, D, device=dev).to(torch.bfloat16)
        (k8, k), (v8, v) = fp8((bh_kv, nk, D), KS), fp8((bh_kv, nk, D), VS)
        oa, ob, oc = (torch.empty_like(q) for _ in range(3))
        kw8 = dict(k_scale=KS, v_scale=VS, scale=SCALE)
        if page:   # the same cache as pages of `page` rows of one head under a shuffled table
            table = torch.randperm(bh_kv * (nk // page), device=dev).to(torch.int32).reshape(bh_kv, nk // page)
            where = table.flatten().long()
            kp8, vp8 = (torch.empty(bh_kv * (nk // page), page, D, dtype=torch.uint8, device=dev) for _ in range(2))
            kp, vp = (torch.empty(bh_kv * (nk // page), page, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
            kp8[where], vp8[where] = k8.view(torch.uint8).view(-1, page, D), v8.view(torch.uint8).view(-1, page, D)
            kp[where], vp[where] = k.view(-1, page, D), v.view(-1, page, D)
            kp8, vp8 = kp8.view(F8), vp8.view(F8)
            ws = torch.empty(max(fa.workspace_bytes_paged(bh_kv, 1, group, nq, nk, D, causal), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: fa.prefill_paged_fp8(q, kp8, vp8, table, causal, out=oa, **kw8),
                    "b": lambda: fa.forward_paged_fp8(q, kp8, vp8, table, causal, out=ob, workspace=ws, **kw8),
                    "c": lambda: fa.prefill_paged(q, kp, vp, table, causal, scale=SCALE * KS, out=oc)}
        else:
            ws = torch.empty(max(fa.workspace_bytes_kv(bh_kv, group, nq, nk, D, causal), 256), dtype=torch.uint8, device=dev)
            arms = {"a": lambda: fa.prefill_kv_fp8(q, k8, v8, causal, out=oa, **kw8),
                    "b": lambda: fa.forward_kv_fp8(q, k8, v8, causal, out=ob, workspace=ws, **kw8),
                    "c": lambda: fa.prefill_kv(q, k, v, causal, scale=SCALE * KS, out=oc)}
        arms["a"](), arms["b"]()
        torch.cuda.synchronize()
        diff = float((oa.float() - ob.float()).abs().max())
        assert diff < TOL_BF16, f"{label} nq {nq} nk {nk}: the outputs of a and b differ by {diff:.3e}"
        r = measure(arms)
        say(f"| {label} | {bh_kv} | {group} | {nq} | {nk} | {bh_kv * -(-group * nq // 256)} | {fmt(r['a'], flop)} | {fmt(r['b'], flop)} | {fmt(r['c'], flop)} | "
            f"{r['a'][0] / r['b'][0]:.3f} | {beyond(r['a'], r['b'])} | {r['a'][0] / r['c'][0]:.3f} | {beyond(r['a'], r['c'])} |")
        del q, k8, v8, k, v, oa, ob, oc

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
