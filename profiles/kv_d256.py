"""Measurements behind docs/kv_d256.md: the head-dim-256 decode kernel (libflashattn_amd_kv256.so) against its two yardsticks, by the method of
profiles/kv_decode.py -- warmed launches on one stream, device events, K/V buffers rotated beyond the Infinity Cache, arms alternated, three
repeats, medians with their spread.

  a  fa_kv256_forward, nq = 1, group 8, d = 256
  b  fa_kv_stream_read on the same buffers viewed as (bh_kv, 2 nk, 128): byte for byte the same read (the floor)
  c  fa_kv_forward at d = 128 on that view: another function of the data, used only as a time
Then a paged row (pages of 16, identity table), a windowed row (4096 keys of 16384), and the largest error of every output kind on the shapes
and seeds of tests/test_gpu_kv256.py, at d = 256 and at d = 128.

    python profiles/kv_d256.py [--out FILE] [--quick]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP, REPEATS = 8, 3
SHAPES = [(8, 8192), (64, 8192), (512, 4096), (512, 16384)]   # bh_kv, nk at d = 256
ROTATE_BYTES = 1 << 30   # K + V over all rotated buffers: four times the Infinity Cache
PARITY = [(2, 1, 1, 1), (3, 4, 1, 31), (2, 8, 1, 33), (1, 8, 1, 257), (2, 4, 5, 1000), (1, 4, 33, 700), (2, 1, 40, 24)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="rehearsal: the two small shapes, few launches")
    a = ap.parse_args()

    import numpy as np
    import torch
    import flashattention_c_amd as fa
    from flashattention_c_amd import _cabi_kv, _cabi_kv256
    from oracle import oracle as orc
    from tests.kv_reference import attention_kv
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    BF16 = _cabi_kv.FA_DTYPE_BF16
    KV, W = _cabi_kv.lib(), _cabi_kv256.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn, launches):
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

    def measure(arms, launches):
        """arms alternated within a repeat; median and (min, max) of the repeats, microseconds"""
        t = {n: [] for n in arms}
        for _ in range(REPEATS):
            for n, fn in arms.items():
                t[n].append(timed(fn, launches))
        return {n: (statistics.median(x), min(x), max(x)) for n, x in t.items()}

    def fmt(x):
        return f"{x[0]:9.1f} ({x[1]:.1f} .. {x[2]:.1f})"

    say("| bh_kv x nk (d = 256) | K+V GB | a: kv256 us | b: stream read us | c: kv d=128 us | a/b | a/c | a GB/s |")
    say("|---|---|---|---|---|---|---|---|")
    for bh, nk in (SHAPES[:2] if a.quick else SHAPES):
        kv_bytes = 2 * bh * nk * 256 * 2
        nbuf = max(1, -(-ROTATE_BYTES // kv_bytes))
        launches = 10 if a.quick else int(min(200, max(10, 60e9 // kv_bytes)))
        k = torch.empty(nbuf, bh, nk, 256, dtype=torch.bfloat16, device=dev).normal_()
        v = torch.empty(nbuf, bh, nk, 256, dtype=torch.bfloat16, device=dev).normal_()
        q = {d: torch.randn(bh * GROUP, 1, d, device=dev).to(torch.bfloat16) for d in (128, 256)}
        o = {d: torch.empty(bh * GROUP, 1, d, dtype=torch.bfloat16, device=dev) for d in (128, 256)}
        sink = torch.zeros(1024, dtype=torch.int32, device=dev)
        need_a = int(W.fa_kv256_workspace_bytes(bh, GROUP, 1, nk, 256, 0, BF16, -1))
        need_c = int(KV.fa_kv_workspace_bytes(bh, GROUP, 1, 2 * nk, 128, 0, BF16))
        ws = torch.empty(max(need_a, need_c, 256), dtype=torch.uint8, device=dev)

        def arm_a(i, window=-1):
            j = i % nbuf
            rc = W.fa_kv256_forward(q[256].data_ptr(), k[j].data_ptr(), v[j].data_ptr(), o[256].data_ptr(), None, bh, GROUP, 1, nk, nk, None, 256, 0.0625, 0, BF16,
                                    window, ws.data_ptr() if need_a else None, need_a, stream())
            assert rc == 0, W.fa_kv256_last_error()

        def arm_b(i):
            j = i % nbuf
            assert KV.fa_kv_stream_read(k[j].data_ptr(), v[j].data_ptr(), bh, 2 * nk, 2 * nk, 128, sink.data_ptr(), stream()) == 0

        def arm_c(i):
            j = i % nbuf
            rc = KV.fa_kv_forward(q[128].data_ptr(), k[j].data_ptr(), v[j].data_ptr(), o[128].data_ptr(), None, bh, GROUP, 1, 2 * nk, 2 * nk, None, 128, 0.088, 0,
                                  BF16, ws.data_ptr() if need_c else None, need_c, stream())
            assert rc == 0, KV.fa_kv_last_error()

        r = measure({"a": arm_a, "b": arm_b, "c": arm_c}, launches)
        say(f"| {bh} x {nk} | {kv_bytes / 1e9:.3f} | {fmt(r['a'])} | {fmt(r['b'])} | {fmt(r['c'])} | {r['a'][0] / r['b'][0]:.3f} | {r['a'][0] / r['c'][0]:.3f} | "
            f"{kv_bytes / r['a'][0] / 1e3:.0f} |")

        if (bh, nk) == (64, 8192):   # the paged row: the same cache as pages of 16 rows under an identity table
            table = torch.arange(bh * (nk // 16), dtype=torch.int32, device=dev).reshape(bh, nk // 16)
            qd, od = q[256], o[256]
            wsp = torch.empty(max(fa.workspace_bytes_paged(bh, 1, GROUP, 1, nk, 256), 256), dtype=torch.uint8, device=dev)

            def arm_p(i):
                j = i % nbuf
                fa.forward_paged(qd, k[j].view(-1, 16, 256), v[j].view(-1, 16, 256), table, False, scale=0.0625, out=od, workspace=wsp)

            def arm_a_py(i):
                j = i % nbuf
                fa.forward_kv(qd, k[j], v[j], False, scale=0.0625, out=od, workspace=wsp)
            rp = measure({"paged": arm_p, "contiguous": arm_a_py}, launches)
            paged_line = f"paged, pages of 16, identity table, {bh} x {nk}, through fa.forward_paged / fa.forward_kv: paged {fmt(rp['paged'])} us, contiguous {fmt(rp['contiguous'])} us"
        del k, v

    say()
    say(paged_line)
    if not a.quick:   # the windowed row: 4096 keys of 16384
        bh, nk, w = 64, 16384, 4095
        kv_bytes = 2 * bh * nk * 256 * 2
        nbuf = max(1, -(-ROTATE_BYTES // kv_bytes))
        k = torch.empty(nbuf, bh, nk, 256, dtype=torch.bfloat16, device=dev).normal_()
        v = torch.empty(nbuf, bh, nk, 256, dtype=torch.bfloat16, device=dev).normal_()
        qd = torch.randn(bh * GROUP, 1, 256, device=dev).to(torch.bfloat16)
        od = torch.empty_like(qd)
        wsw = torch.empty(max(fa.workspace_bytes_kv(bh, GROUP, 1, nk, 256), 256), dtype=torch.uint8, device=dev)
        rw = measure({"window": lambda i: fa.forward_kv(qd, k[i % nbuf], v[i % nbuf], True, scale=0.0625, out=od, workspace=wsw, window_left=w),
                      "full": lambda i: fa.forward_kv(qd, k[i % nbuf], v[i % nbuf], True, scale=0.0625, out=od, workspace=wsw)}, 100)
        say(f"window of 4096 keys on {bh} x {nk}, causal, through fa.forward_kv: windowed {fmt(rw['window'])} us, no window {fmt(rw['full'])} us")
        del k, v

    say()
    say("largest |error| against the fp64 reference over the parity shapes of tests/test_gpu_kv256.py (seeds 61-63, causal and not, scales 1 and 1/16)")
    say("| d | fp32 O | LSE | bf16 O |")
    say("|---|---|---|---|")
    for d in (256, 128):
        worst = {"f32": 0.0, "lse": 0.0, "bf16": 0.0}
        for bh_kv, group, nq, nk in PARITY:
            g = lambda seed, *s: orc.round_to_bf16(torch.randn(*s, generator=torch.Generator().manual_seed(seed)).numpy())  # noqa: E731
            qn, kn, vn = g(61, bh_kv * group, nq, d), g(62, bh_kv, nk, d), g(63, bh_kv, nk, d)
            qd, kd, vd = (torch.from_numpy(np.ascontiguousarray(t)).to(torch.bfloat16).to(dev) for t in (qn, kn, vn))
            for causal in (False, True):
                for scale in (1.0, 1.0 / 16):
                    ref, lse_ref = attention_kv(qn, kn, vn, None, causal, scale)
                    fin = np.isfinite(lse_ref)
                    for odt, kind in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                        oo, lse = fa.forward_kv(qd, kd, vd, causal, scale=scale, out_dtype=odt, return_lse=True)
                        worst[kind] = max(worst[kind], float(np.abs(oo.float().cpu().numpy() - ref).max()))
                        if fin.any():
                            worst["lse"] = max(worst["lse"], float(np.abs(lse.cpu().numpy()[fin] - lse_ref[fin]).max()))
        say(f"| {d} | {worst['f32']:.3e} | {worst['lse']:.3e} | {worst['bf16']:.3e} |")

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
