"""CPU: libuwu_hip.so builds, loads, and exports every symbol include/uwu_hip.h declares (no compute)."""
import ctypes
import os
import re

from tests.conftest import ROOT


def header_symbols():
    src = open(os.path.join(ROOT, "include", "uwu_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uwu_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_all_header_symbols():
    from uwudiff_amd import build, lib

    build.build(verbose=False)
    cd = ctypes.CDLL(lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(cd, s)]
    assert not missing, f"not exported: {missing}"
    # the ctypes table binds exactly the header's entry points
    assert sorted(lib.exported_symbols()) == syms
    l = lib.load()
    assert l.uwu_version() >= 1
    assert isinstance(l.uwu_last_error(), bytes)


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing elsewhere."""
    import pytest
    import torch

    from uwudiff_amd import lib

    with pytest.raises(lib.UwuError):
        lib.ptr(torch.zeros(4))


def test_product_does_not_import_oracle():
    bad = []
    for pkg in ("uwudiff_amd", "duwu", "tools", "test_scripts"):
        for dp, _, fs in os.walk(os.path.join(ROOT, pkg)):
            for f in fs:
                if f.endswith(".py"):
                    s = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", s, flags=re.M):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_ctypes_arity_matches_header():
    """Every ctypes signature has exactly as many parameters as the C prototype in include/uwu_hip.h."""
    from uwudiff_amd import lib

    src = open(os.path.join(ROOT, "include", "uwu_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\b(uwu_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    for name, (_, args) in lib._SIGS.items():
        params = protos[name].strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(args), f"{name}: header has {n} params, ctypes table has {len(args)}"


def test_counted_vmcnt_kernels_do_not_spill(tmp_path):
    """gemm_as_kernel hand-counts its vector-memory operations (s_waitcnt vmcnt(N)); a register spill would add scratch
    accesses to that sequence.  Checked on the kernel metadata of the built library's gfx950 code objects (no GPU needed)."""
    import os
    import re
    import subprocess

    import pytest

    from uwudiff_amd import build

    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("LLVM binary utilities not available")
    if not os.path.exists(build.LIB):
        build.build()
    fat = tmp_path / "fat.bin"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", build.LIB, str(tmp_path / "unused.so")], check=True,
                   capture_output=True)
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, "no offload bundles in the library"
    seen = 0
    for i, st in enumerate(starts):  # one bundle per translation unit
        part = tmp_path / f"bundle{i}.bin"
        part.write_bytes(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = tmp_path / f"co{i}.o"
        subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={part}", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True)
        if not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([tools[2], "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*gemm_as_kernel\S*)", notes):
            seen += 1
            tail = notes[m.end():m.end() + 1500]
            sp = re.search(r"\.vgpr_spill_count:\s*(\d+)", tail)
            assert sp and int(sp.group(1)) == 0, (m.group(1), tail[:300])
    assert seen >= 3, seen


# Environment switches the library may read: the ones the GPU tests set to pin a kernel against its reference kernel, and the
# side-stream count of the DiT step.  A name outside this list is a tuning or timing-only switch left in a launch path.
KEPT_SWITCHES = {
    "UWU_GEMM_AS", "UWU_GEMM_AS_BIAS", "UWU_GEMM_M64", "UWU_GEMM_WIDE", "UWU_GEMM_BIG", "UWU_GEMM_TR", "UWU_GEMM_TRW",
    "UWU_GEMM_R3", "UWU_GEMM_P8", "UWU_GEMM_P8N", "UWU_GEMM_P8F", "UWU_GEMM_P8F_PART", "UWU_F8_EMIT", "UWU_LN_ROW16",
    "UWU_ATTN_P256", "UWU_ATTN_P256F", "UWU_ATTN_P256_D72", "UWU_ATTN_P256F_D72", "UWU_DIT_SIDE_STREAMS",
}


def test_library_reads_only_the_kept_switches():
    """Every UWU_* string in libuwu_hip.so that include/uwu_hip.h does not declare is one of KEPT_SWITCHES (no GPU needed)."""
    from uwudiff_amd import build

    if not os.path.exists(build.LIB):
        build.build()
    found = {m.decode() for m in re.findall(rb"UWU_[A-Z0-9_]+", open(build.LIB, "rb").read())}
    declared = set(re.findall(r"\bUWU_[A-Z0-9_]+\b", open(os.path.join(ROOT, "include", "uwu_hip.h")).read()))
    assert found - declared == KEPT_SWITCHES
