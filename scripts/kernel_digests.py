"""Per-symbol digests of the device code of .hip files (CPU only: cross-compiles, runs nothing).

Each file is compiled with the _build.py flags plus --cuda-device-only --no-gpu-bundle-output.
One line per device symbol: its name, the sha256 (16 hex digits) of its instruction encodings
(llvm-objdump -d) and, for a kernel, vgpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count,
group_segment_fixed_size and private_segment_fixed_size (llvm-readelf --notes).  An out-of-line
device function has no such record and may exist once per file: its line ends with the file.
With two file lists (separated by --) the kernels whose lines differ are printed, then the counts.

    python scripts/kernel_digests.py csrc/f110_post.hip
    python scripts/kernel_digests.py parent/csrc/*.hip -- csrc/*.hip

The second form, over a checkout of the parent commit and this tree, is the proof that a change of
the headers alone (moving text between csrc/*.h, changing includes) left every kernel as it was.

--layout-free (first argument) hashes the instruction text instead of the encodings, with the
literal of every `s_add_u32 sN, sN, 0x...` masked: those are the pc-relative address computations
(s_getpc_b64 + offset of a constant table or an out-of-line function), which move with the file's
layout -- a kernel added to the file, a longer mangled name -- while the kernel's code does not.

    python scripts/kernel_digests.py --layout-free parent/csrc/f110_agents.hip -- csrc/f110_agents.hip
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f110_gymnasium_ros2_jazzy_amd import _build  # noqa: E402

META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def llvm(tool):
    return os.path.join(os.path.dirname(os.path.dirname(_build.hipcc())), "llvm", "bin", tool)


LAYOUT_FREE = False


def digests(path, tmp):
    """(kernels {name: line}, device functions [line]) of one .hip file's code object."""
    co = os.path.join(tmp, os.path.basename(path) + ".co")
    subprocess.check_call([_build.hipcc()] + _build.FLAGS +
                          ["--cuda-device-only", "--no-gpu-bundle-output", path, "-o", co])
    code, sym = {}, None
    for ln in subprocess.check_output([llvm("llvm-objdump"), "-d", co], text=True).splitlines():
        head = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if head:
            sym = head.group(1)
            code[sym] = hashlib.sha256()
        elif sym and "//" in ln:  # "\tinstruction // address: encoding words"
            if LAYOUT_FREE:
                text = re.sub(r"(s_add_u32 s\d+, s\d+, )0x[0-9a-f]+", r"\1<pcrel>", ln.split("//")[0].strip())
                code[sym].update(text.encode() + b"\n")
            else:
                code[sym].update(ln.split("//")[1].split(":", 1)[1].strip().encode())
    records = []  # amdhsa.kernels: "  - .key: value" opens a kernel's record, "    .key: value" continues it
    for ln in subprocess.check_output([llvm("llvm-readelf"), "--notes", co], text=True).splitlines():
        kv = re.match(r"  ([- ]) \.(\w+):\s*(\S*)\s*$", ln)
        if kv and kv.group(1) == "-":
            records.append({})
        if kv and records:
            records[-1][kv.group(2)] = kv.group(3)
    meta = {r["name"]: r for r in records if r.get("name") in code}
    kernels = {s: " ".join([s, code[s].hexdigest()[:16]] + [f"{k}={m.get(k, '?')}" for k in META])
               for s, m in meta.items()}
    funcs = [f"{s} {h.hexdigest()[:16]} ({os.path.basename(path)})" for s, h in code.items() if s not in meta]
    return kernels, funcs


def side(files, tmp):
    kernels, funcs = {}, []
    for f in files:
        k, fn = digests(f, tmp)
        kernels.update(k)
        funcs += fn
    return kernels, funcs


def main(argv):
    global LAYOUT_FREE
    if argv and argv[0] == "--layout-free":
        LAYOUT_FREE, argv = True, argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)
    with tempfile.TemporaryDirectory() as tmp:
        a, fa = side(argv[:cut], tmp)
        if cut == len(argv):
            print("\n".join([a[s] for s in sorted(a)] + sorted(fa)))
            return
        b, _ = side(argv[cut + 1:], tmp)
    for s in sorted(set(a) | set(b)):
        if a.get(s) != b.get(s):
            print("<", a.get(s, s + " (absent)"))
            print(">", b.get(s, s + " (absent)"))
    same = sum(1 for s in set(a) & set(b) if a[s] == b[s])
    print(f"kernels: {len(a)} / {len(b)}, same names: {set(a) == set(b)}, identical: {same}, "
          f"differing: {len(set(a) | set(b)) - same}")


if __name__ == "__main__":
    main(sys.argv[1:])
