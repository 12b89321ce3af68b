"""The reader of the kernel-resources tests (test_qs_kernel_resources.py: the nine kernels over qs_body, a table, and four older files of one kernel each; test_side_kernel_resources.py
and test_words_kernel_resources.py: k_search_side and k_search_words): what the compiler made of every kernel in the built gfx950 code objects, read the
way tools/kernel_resources.py reads them (llvm-readelf --notes on the code objects bundled in libfpx.so, or in build/fpx_search.o).
A helper module like fpx_testlib.py: no test, no fixture."""
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "acoustid-index_amd")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def _notes(path):
    """llvm-readelf --notes of every gfx950 code object bundled in `path` (an object file, or the shared library: a bundle per object)"""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    assert objcopy and bundler and readelf, "the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf) were not found"
    magic, out = b"__CLANG_OFFLOAD_BUNDLE__", []
    with tempfile.TemporaryDirectory() as d:
        fat, co, one = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co"), os.path.join(d, "one.bin")
        subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", path, os.path.join(d, "copy")], check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), data)]
        for a, b in zip(starts, starts[1:] + [len(data)]):
            with open(one, "wb") as fh:
                fh.write(data[a:b])
            subprocess.run([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={one}", f"--output={co}"],
                           check=True, capture_output=True)
            if os.path.getsize(co):
                out.append(subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout)
    return "\n".join(out)


@functools.lru_cache(maxsize=None)
def _read():
    """{mangled name: {field: int}} of the built artefact, None where nothing is built; once per process"""
    lib = os.path.join(PKG, "libfpx.so")
    if not glob.glob(os.path.join(PKG, "build", "*.o")) and not os.path.exists(lib):
        return None
    # (the library is what runs; an object file only where there is no library)
    notes = _notes(lib if os.path.exists(lib) else os.path.join(PKG, "build", "fpx_search.o"))
    found = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n\s+- \.agpr_count:|\namdhsa\.target|\Z)", notes, flags=re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        figures = {f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1)) for f in FIELDS}
        # (a template's instantiation may be in the code objects of several object files: the same kernel, the same figures)
        assert found.setdefault(name, figures) == figures, f"{name}: twice in the built code objects, with different figures"
    return found


def kernels():
    """{mangled name: {field: int} for FIELDS} for every kernel of libfpx.so, else of build/fpx_search.o; skips the calling test where
    neither is built"""
    found = _read()
    if found is None:
        pytest.skip("nothing built: neither libfpx.so nor build/*.o")
    return found
