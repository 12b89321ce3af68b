"""What the compiler made of k_search_query (csrc/fpx_qsearch.hpp), read from the built code objects the way tools/kernel_resources.py
reads them (llvm-readelf --notes on the gfx950 code object in build/fpx_search.o, or in libfpx.so): conditions on registers, spills and
scratch that hold for all sixteen instantiations (8 / 16 columns x QS x MEM x FILT) -- no GPU needed.

* an unfiltered instantiation spills no vector register and has no scratch segment (the once-per-query kernel arguments are read from
  the kernel-argument segment where they are used, the columns' hash bounds stay in LDS);
* a filtered one has no more scratch than before that change: 88 bytes at 16 columns, 24 at 8;
* none is above 128 vector registers (four waves per SIMD) or 106 scalar ones;
* the static LDS stays what it was (784 / 848 bytes): with the kernel's dynamic 39 KB four workgroups share a CU's 160 KB."""
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


def _kernels():
    objs = sorted(glob.glob(os.path.join(PKG, "build", "*.o")))
    lib = os.path.join(PKG, "libfpx.so")
    search_o = os.path.join(PKG, "build", "fpx_search.o")
    if not objs and not os.path.exists(lib):
        pytest.skip("nothing built: neither libfpx.so nor build/*.o")
    # (the library is what runs; an object file only where there is no library)
    notes = _notes(lib if os.path.exists(lib) else search_o)
    found = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n\s+- \.agpr_count:|\namdhsa\.target|\Z)", notes, flags=re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb([01])ELb([01])EEEv", name)
        if t:
            key = (int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))), bool(int(t.group(4))))       # NS, QS, MEM, FILT
            found[key] = {f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1)) for f in FIELDS}
    return found


@pytest.fixture(scope="module")
def kernels():
    k = _kernels()
    assert len(k) == 16, f"k_search_query: {len(k)} instantiations in the built code object, sixteen expected: {sorted(k)}"
    return k


def test_sixteen_instantiations(kernels):
    assert sorted(kernels) == sorted((ns, qs, mem, filt) for ns in (8, 16) for qs in (False, True) for mem in (False, True) for filt in (False, True))


def test_unfiltered_kernels_do_not_spill_vector_registers(kernels):
    for key, r in kernels.items():
        if not key[3]:
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (key, r)


def test_filtered_kernels_have_no_more_scratch_than_before(kernels):
    for key, r in kernels.items():
        if key[3]:
            assert r["private_segment_fixed_size"] <= (88 if key[0] == 16 else 24), (key, r)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(kernels):
    for key, r in kernels.items():
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= (848 if key[3] else 784), (key, r)

