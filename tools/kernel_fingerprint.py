"""Fingerprint of every gfx950 kernel in a built library or in object files (no GPU needed).

    python tools/kernel_fingerprint.py uwudiff_amd/libuwu_hip.so            > after.txt
    python tools/kernel_fingerprint.py path/to/other/build/_obj/*.o         > before.txt
    diff before.txt after.txt

One sorted line per kernel: the mangled name, the SHA-256 of the function's bytes in .text, and the register / spill / LDS /
scratch figures of its metadata note.  Two builds whose outputs are equal as text hold the same multiset of kernels (none
gained, lost or compiled twice) with the same machine code -- the check for a change that only moves source between files.
A library and the objects it was linked from give the same lines, so either may stand for a build.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size")


def tool(name, *args, text=True):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=text).stdout


def code_objects(path, tmp):
    """The gfx950 code objects embedded in a host object or shared library: one per translation unit (none in plain C++ objects)."""
    if ".hip_fatbin" not in tool("llvm-readelf", "-S", "--wide", path):
        return
    fat = os.path.join(tmp, "fat.bin")
    if os.path.exists(fat):
        os.remove(fat)
    tool("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path, os.path.join(tmp, "unused"))
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    for i, st in enumerate(starts):
        part, co = os.path.join(tmp, "bundle.bin"), os.path.join(tmp, "co.o")
        with open(part, "wb") as f:
            f.write(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        if os.path.exists(co):
            os.remove(co)
        tool("clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}", f"--output={co}", f"--targets={TARGET}")
        if os.path.getsize(co):
            yield co


def kernels(co):
    """(name, sha256 of the code, metadata fields) of every kernel of one code object."""
    notes = tool("llvm-readelf", "--notes", co)
    meta = {}
    if "amdhsa.kernels:" not in notes:
        return
    section = notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0]  # a list of maps; a kernel's own keys sit at 4 spaces
    for block in re.split(r"^  - ", section, flags=re.M)[1:]:
        top = dict(re.findall(r"^    (\.\w+):\s+(\S+)\s*$", "    " + block, flags=re.M))
        meta[top[".name"]] = top
    text = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", tool("llvm-readelf", "-S", "--wide", co))
    addr, off, size = (int(x, 16) for x in text.groups())
    funcs = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\d+\s+(\S+)\s*$", tool("llvm-readelf", "-s", "--wide", co),
                         flags=re.M):
        funcs[m.group(3)] = (int(m.group(1), 16), int(m.group(2)))
    blob = open(co, "rb").read()
    for name, top in meta.items():
        value, length = funcs[name]
        assert addr <= value and value + length <= addr + size, name
        code = blob[off + value - addr:off + value - addr + length]
        yield name, hashlib.sha256(code).hexdigest(), [top[f] for f in FIELDS]


def main(paths):
    if not paths:
        sys.exit(__doc__)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for path in paths:
            for co in code_objects(path, tmp):
                for name, digest, fields in kernels(co):
                    lines.append(" ".join([name, digest, *(f"{f[1:]}={v}" for f, v in zip(FIELDS, fields))]))
    print("\n".join(sorted(lines)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
