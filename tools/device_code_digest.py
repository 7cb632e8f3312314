"""Digest of the device code of every kernel: each csrc/*.hip is compiled with the build's own flags (__graft_entry__.FLAGS) plus
--cuda-device-only -S; one line per kernel, sorted by demangled name and without a file column, carries the .amdhsa resource fields and a
sha256 (64 bits of it) of the kernel's instruction text (comments, .p2align / .loc / .cfi / .file lines dropped, .LBB labels renumbered in order of
appearance).  Two trees whose outputs are byte-identical run the same device code, wherever a kernel lives: the check of a refactor that
moves kernels between files (build container, no GPU).  Usage: python tools/device_code_digest.py [file.hip ...] > profiles/rNN_device_code.txt"""
import glob
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import FLAGS, HIPCC  # noqa: E402

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
DROP = re.compile(r"\s*\.(p2align|loc|cfi_\w+|file)\b")


def asm(f):
    return subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", f, "-o", "-"], capture_output=True, text=True, check=True).stdout


def kernels(text):
    """(mangled name, resource fields, normalised body) of every kernel of one assembly file"""
    res = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        res[m.group(1)] = {k: v for k, v in re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)) if k in FIELDS}
    for name in res:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        lines = [re.sub(r"\s*;.*", "", ln).rstrip() for ln in body.splitlines()]
        body = "\n".join(ln for ln in lines if ln.strip() and not DROP.match(ln))
        labels = {}
        body = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".LBB%d" % len(labels)), body)
        yield name, res[name], body


if __name__ == "__main__":
    files = sys.argv[1:] or sorted(glob.glob(os.path.join(ROOT, "adamml_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(8) as pool:
        found = [k for text in pool.map(asm, files) for k in kernels(text)]
    names = subprocess.run(["c++filt"], input="\n".join(k[0] for k in found), capture_output=True, text=True, check=True).stdout.splitlines()
    # (short rows, since the outputs get committed: no "void", namespace or argument list in a name, the field names once, 64 bits of the hash)
    print("%d kernels: name | %s | sha256 of the instruction text, first 16 hex digits" % (len(found), " ".join(FIELDS)))
    rows = ["%s | %s | %s" % (re.sub(r"\(.*\)$", "", re.sub(r"^void |\(anonymous namespace\)::", "", name)), " ".join(r.get(k, "-") for k in FIELDS),
                              hashlib.sha256(body.encode()).hexdigest()[:16]) for name, (_, r, body) in zip(names, found)]
    print("\n".join(sorted(rows)))
