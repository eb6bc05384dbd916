"""CPU: the instruction profile of every kernel of the five KV-cache libraries (libflashattn_amd_kv.so, _paged.so, _kv8.so, _kvw.so, _kvw8.so)
against tests/golden/kv_kernel_profile.txt.  The lines of the first three were recorded from a build of the commit before their decode loops,
merges and validators were folded into shared headers (csrc/fa_kv_decode_core.h, fa_kv_combine_kernel.h, fa_kv_host.h); the lines of the two
windowed libraries (16 decode kernels + 2 merge kernels each) from a build of the commit before their build rules moved into one table, with the
other 39 lines coming out unchanged.

Sharing source text lets hipcc renumber scalar registers and move scalar / address instructions, so neither the bytes of a code object nor
its instruction total are held.  What a change of these kernels must not move is held, per mangled kernel name:
    the set of kernels; LDS bytes and scratch bytes (equal); VGPRs + AGPRs (not above the golden);
    the number of instructions whose mnemonic starts with one of PREFIXES, over the kernel's whole body (equal);
    the sorted list of the vmcnt(N) immediates of its s_waitcnt instructions (equal).

Re-record (after a change that is MEANT to move one of these, with the reason in the commit message):
    python flashattention.c_amd/build.py && python -m tests.test_kv_code_profile --record
"""
import os
import re
import sys
import tempfile

import pytest

from flashattention_c_amd import _cabi_kv, _cabi_kv8, _cabi_kvw, _cabi_kvw8, _cabi_paged
from tests import codeobj
from tests.conftest import GOLDEN_DIR

GOLDEN = os.path.join(GOLDEN_DIR, "kv_kernel_profile.txt")
LIBS = (("kv", _cabi_kv.LIB_PATH), ("paged", _cabi_paged.LIB_PATH), ("kv8", _cabi_kv8.LIB_PATH), ("kvw", _cabi_kvw.LIB_PATH),
        ("kvw8", _cabi_kvw8.LIB_PATH))
PREFIXES = ("v_mfma", "global_load", "ds_read", "ds_write", "global_store", "v_exp", "v_permlane", "v_cvt_pk", "s_barrier")


def _bodies(disassembly):
    """symbol -> the mnemonic-and-operands lines between its label and the next one"""
    out, cur = {}, None
    for ln in disassembly.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t"):
            cur.append(ln.split("//")[0].strip())
    return out


def profile_of(lib_path, outdir):
    """mangled name -> one golden line (without the library tag)"""
    kernels = codeobj.kernels_of(lib_path, outdir)
    bodies = {}
    for co in sorted({k.code_object for k in kernels.values()}):
        bodies.update(_bodies(codeobj.disassemble(co)))
    lines = {}
    for name, k in kernels.items():
        body = bodies[name]
        assert len(body) > 10, name
        counts = [sum(1 for ins in body if ins.split()[0].startswith(p)) for p in PREFIXES]
        vmcnt = sorted(int(n) for ins in body if ins.startswith("s_waitcnt") for n in re.findall(r"vmcnt\((\d+)\)", ins))
        lines[name] = " ".join([f"lds={k.lds}", f"scratch={k.scratch}", f"regs={k.vgprs + k.agprs}"] + [f"{p}={c}" for p, c in zip(PREFIXES, counts)] +
                               ["vmcnt=" + (",".join(map(str, vmcnt)) or "-")])
    return lines


def current(outdir):
    return {f"{tag} {name}": line for tag, path in LIBS for name, line in profile_of(path, os.path.join(outdir, tag)).items()}


def _fields(line):
    return dict(f.split("=", 1) for f in line.split())


def test_every_kv_kernel_keeps_its_instruction_profile(tmp_path):
    for tag, _ in LIBS:
        os.makedirs(tmp_path / tag)
    want = {}
    for ln in open(GOLDEN).read().splitlines():
        if ln and not ln.startswith("#"):
            tag, name, rest = ln.split(" ", 2)
            want[f"{tag} {name}"] = rest
    have = current(str(tmp_path))
    assert set(have) == set(want), sorted(set(have) ^ set(want))
    assert len(have) == 11 + 10 + 18 + 18 + 18   # kv, paged, kv8, kvw, kvw8
    bad = []
    for key in sorted(want):
        w, h = _fields(want[key]), _fields(have[key])
        assert set(w) == set(h) == {"lds", "scratch", "regs", "vmcnt", *PREFIXES}
        moved = [f"{f}: {w[f]} -> {h[f]}" for f in w if (int(h[f]) > int(w[f]) if f == "regs" else h[f] != w[f])]
        if moved:
            bad.append(f"{key}\n    " + "\n    ".join(moved))
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for tag, _ in LIBS:
            os.makedirs(os.path.join(tmp, tag))
        rows = current(tmp)
    with open(GOLDEN, "w") as f:
        f.write("# The instruction profile of every kernel of the KV-cache libraries: tests/test_kv_code_profile.py says what is held and how.\n"
                "# Re-record: python flashattention.c_amd/build.py && python -m tests.test_kv_code_profile --record\n"
                "# <library> <mangled kernel> lds scratch regs(vgpr + agpr) <count per mnemonic prefix> <sorted vmcnt(N) immediates>\n")
        for key in sorted(rows):
            f.write(f"{key} {rows[key]}\n")
    print(f"{len(rows)} kernels -> {GOLDEN}")
