"""CPU: gemm_trw_kernel (hand-counted vmcnt waits, ~230 of its 256 VGPRs) must not spill in the built library's gfx950 code objects.

The grouped launch selects its member with scalar registers only; a spill would put scratch accesses into the counted
vector-memory sequence of the K loop."""
import os
import re
import subprocess

import pytest


def test_gemm_trw_kernels_do_not_spill(tmp_path):
    from uwudiff_amd import build

    llvm = "/opt/rocm/lib/llvm/bin"
    objcopy, bundler, readelf = (os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    if not all(os.path.exists(t) for t in (objcopy, bundler, readelf)):
        pytest.skip("LLVM binary utilities not available")
    if not os.path.exists(build.LIB):
        build.build()
    fat = tmp_path / "fat.bin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", build.LIB, str(tmp_path / "unused.so")], check=True,
                   capture_output=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    assert starts, "no offload bundles in the library"
    seen = 0
    for i, st in enumerate(starts):  # one bundle per translation unit
        part = tmp_path / f"bundle{i}.bin"
        part.write_bytes(blob[st:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = tmp_path / f"co{i}.o"
        subprocess.run([bundler, "--unbundle", "--type=o", f"--input={part}", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True)
        if not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        # amdhsa.kernels is a YAML list: one "  - .key: value" line opens a kernel's block, its other keys follow indented
        for block in re.split(r"^\s*- (?=\.)", notes, flags=re.M)[1:]:
            meta = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", block, flags=re.M))
            if "gemm_trw_kernel" not in meta.get("name", ""):
                continue
            seen += 1
            for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
                assert int(meta[key]) == 0, (meta["name"], key, meta[key])
            # 512 threads, one workgroup per CU: two waves per SIMD share its 512 registers
            assert int(meta["vgpr_count"]) <= 256, (meta["name"], meta["vgpr_count"])
    assert seen >= 2, seen  # at least the 192 x 384 and the 384 x 192 instantiation
