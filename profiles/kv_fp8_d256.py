"""Measurements behind docs/kv_fp8_d256.md: the head-dim-256 fp8 decode kernel (libflashattn_amd_kv8_256.so) against its two yardsticks, by the
method of profiles/kv_decode.py -- warmed launches on one stream, device events, K/V buffers rotated over 1 GiB, arms alternated, three
repeats, medians with their spread.  nq = 1, group 8, bf16 output.

  a  fa.forward_kv at d = 256 on the bf16 twin of the cache
  b  fa.forward_kv_fp8 at d = 256
  c  fa_kv_stream_read over the fp8 bytes, viewed as (bh_kv, nk, 128) bf16: byte for byte the same read (the floor)
Then a paged row (pages of 16, identity table, 64 x 8192) and a windowed row (4096 keys of 16384 on 64 slabs).  Before it is timed, every fp8
arm is compared bit for bit with arm a's function on the dequantised cache.  The script asserts b <= a at 512 x 4096 and 512 x 16384.

    python profiles/kv_fp8_d256.py [--out FILE] [--quick]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP, REPEATS, D = 8, 3, 256
SHAPES = [(8, 8192), (64, 8192), (512, 4096), (512, 16384)]   # bh_kv, nk
MUST_NOT_LOSE = [(512, 4096), (512, 16384)]                   # where arm a sits on its own floor and b moves half the bytes
ROTATE_BYTES = 1 << 30
KS, VS, SCALE = 0.013, 1.0, 4.0   # v_scale = 1: the bits compared are the kernel's own.  (The codes are uniform over all 256, so the softmax is
# nearly one-hot and an output can be subnormal; there 0.5 x bf16(x) and bf16(0.5 x) differ, which a first version of this script tripped on.)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="rehearsal: the two small shapes, few launches")
    a = ap.parse_args()

    import numpy as np
    import torch
    import flashattention_c_amd as fa
    from flashattention_c_amd import _cabi_kv
    from tests.kv8_reference import TABLE
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    F8 = torch.float8_e4m3fn
    KV = _cabi_kv.lib()
    lut = torch.from_numpy(np.nan_to_num(TABLE)).to(torch.bfloat16).to(dev)
    folded = float(np.float32(SCALE) * np.float32(KS))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

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
        return f"{x[0]:.1f} ({x[1]:.1f} .. {x[2]:.1f})"

    def caches(nbuf, bh, nk):
        """random fp8 codes without the NaN codes, and their exact bf16 twin (a table look-up, in pieces)"""
        c8 = torch.empty((2, nbuf, bh, nk, D), dtype=torch.uint8, device=dev)
        tw = torch.empty(c8.shape, dtype=torch.bfloat16, device=dev)
        flat8, flat = c8.view(-1), tw.view(-1)
        for at in range(0, flat8.numel(), 1 << 26):   # no operation of torch's over more than 2^26 elements
            x = torch.randint(0, 256, (min(1 << 26, flat8.numel() - at),), dtype=torch.uint8, device=dev)
            x[(x & 0x7F) == 0x7F] = 0x38
            flat8[at:at + (1 << 26)] = x
            flat[at:at + (1 << 26)] = lut[x.long()]
        return c8[0].view(F8), c8[1].view(F8), tw[0], tw[1]

    def same_bits(got, want, what):
        off = got.view(torch.int16) != want.view(torch.int16)
        assert not bool(off.any()), (f"{what}: not the bits of arm a on the dequantised cache ({int(off.sum())} of {off.numel()} elements, first row "
                                     f"{int(off.any(-1).flatten().nonzero()[0])}, NaN in b: {bool(torch.isnan(got.float()).any())})")

    say("| bh_kv x nk (d = 256) | fp8 K+V GB | a: bf16 us | b: fp8 us | c: stream read us | b/a | b/c | b GB/s |")
    say("|---|---|---|---|---|---|---|---|")
    lost = []
    for bh, nk in (SHAPES[:2] if a.quick else SHAPES):
        kv_bytes = 2 * bh * nk * D
        nbuf = max(1, -(-ROTATE_BYTES // (2 * kv_bytes)))   # the bf16 twin fills the 1 GiB; the fp8 bytes rotate over the same count
        launches = 10 if a.quick else int(min(200, max(10, 30e9 // kv_bytes)))
        k8, v8, kb, vb = caches(nbuf, bh, nk)
        q = torch.randn(bh * GROUP, 1, D, device=dev).to(torch.bfloat16)
        oa, ob = torch.empty_like(q), torch.empty_like(q)
        sink = torch.zeros(1024, dtype=torch.int32, device=dev)
        ws = torch.empty(max(fa.workspace_bytes_kv(bh, GROUP, 1, nk, D), 256), dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def arm_a(i):
            fa.forward_kv(q, kb[i % nbuf], vb[i % nbuf], False, scale=folded, out=oa, workspace=ws)

        def arm_b(i):
            fa.forward_kv_fp8(q, k8[i % nbuf], v8[i % nbuf], False, k_scale=KS, v_scale=VS, scale=SCALE, out=ob, workspace=ws)

        def arm_c(i):
            j = i % nbuf
            assert KV.fa_kv_stream_read(k8[j].data_ptr(), v8[j].data_ptr(), bh, nk, nk, 128, sink.data_ptr(), stream) == 0

        arm_a(0), arm_b(0)
        same_bits(ob, oa, f"{bh} x {nk}")
        r = measure({"a": arm_a, "b": arm_b, "c": arm_c}, launches)
        say(f"| {bh} x {nk} | {kv_bytes / 1e9:.3f} | {fmt(r['a'])} | {fmt(r['b'])} | {fmt(r['c'])} | {r['b'][0] / r['a'][0]:.3f} | {r['b'][0] / r['c'][0]:.3f} | "
            f"{kv_bytes / r['b'][0] / 1e3:.0f} |")
        if (bh, nk) in MUST_NOT_LOSE and r["b"][0] > r["a"][0]:
            lost.append(f"{bh} x {nk}: b {fmt(r['b'])} us > a {fmt(r['a'])} us")

        if (bh, nk) == (64, 8192):   # the paged row: the same bytes as pages of 16 rows under an identity table
            table = torch.arange(bh * (nk // 16), dtype=torch.int32, device=dev).reshape(bh, nk // 16)
            op = torch.empty_like(q)

            def arm_p(i):
                j = i % nbuf
                fa.forward_paged_fp8(q, k8[j].view(-1, 16, D), v8[j].view(-1, 16, D), table, False, k_scale=KS, v_scale=VS, scale=SCALE, out=op, workspace=ws)

            arm_p(0), arm_b(0)
            assert torch.equal(op.view(torch.int16), ob.view(torch.int16)), "paged: not the bits of the contiguous entry"
            rp = measure({"paged": arm_p, "contiguous": arm_b}, launches)
            paged_line = (f"paged, pages of 16, identity table, {bh} x {nk}: paged {fmt(rp['paged'])} us, contiguous {fmt(rp['contiguous'])} us, "
                          f"ratio {rp['paged'][0] / rp['contiguous'][0]:.3f}")
        del k8, v8, kb, vb

    say()
    say(paged_line)
    if not a.quick:   # the windowed row: 4096 keys of 16384
        bh, nk, w = 64, 16384, 4095
        nbuf = max(1, -(-ROTATE_BYTES // (4 * bh * nk * D)))
        k8, v8, kb, vb = caches(nbuf, bh, nk)
        q = torch.randn(bh * GROUP, 1, D, device=dev).to(torch.bfloat16)
        oa, ob = torch.empty_like(q), torch.empty_like(q)
        ws = torch.empty(max(fa.workspace_bytes_kv(bh, GROUP, 1, nk, D), 256), dtype=torch.uint8, device=dev)
        arms = {"fp8 window": lambda i: fa.forward_kv_fp8(q, k8[i % nbuf], v8[i % nbuf], True, k_scale=KS, v_scale=VS, scale=SCALE, out=ob, workspace=ws, window_left=w),
                "bf16 window": lambda i: fa.forward_kv(q, kb[i % nbuf], vb[i % nbuf], True, scale=folded, out=oa, workspace=ws, window_left=w),
                "fp8 full": lambda i: fa.forward_kv_fp8(q, k8[i % nbuf], v8[i % nbuf], True, k_scale=KS, v_scale=VS, scale=SCALE, out=ob, workspace=ws)}
        arms["bf16 window"](0), arms["fp8 window"](0)
        same_bits(ob, oa, "window")
        rw = measure(arms, 100)
        say(f"window of 4096 keys on {bh} x {nk}, causal: fp8 windowed {fmt(rw['fp8 window'])} us, bf16 windowed {fmt(rw['bf16 window'])} us "
            f"(ratio {rw['fp8 window'][0] / rw['bf16 window'][0]:.3f}), fp8 without a window {fmt(rw['fp8 full'])} us")

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not lost, "the fp8 call is slower than the bf16 call where it must not be: " + "; ".join(lost)


if __name__ == "__main__":
    main()
