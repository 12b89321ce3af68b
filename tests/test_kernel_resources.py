"""What the compiler made of k_search_query (csrc/fpx_qsearch.hpp), read from the built code objects the way tools/kernel_resources.py
reads them (llvm-readelf --notes on the gfx950 code object in build/fpx_search.o, or in libfpx.so): conditions on registers, spills and
scratch that hold for all sixteen instantiations (8 / 16 columns x QS x MEM x FILT) -- no GPU needed.

* an unfiltered instantiation spills no vector register and has no scratch segment (the once-per-query kernel arguments are read from
  the kernel-argument segment where they are used, the columns' hash bounds stay in LDS);
* a filtered one has no more scratch than before that change: 88 bytes at 16 columns, 24 at 8;
* none is above 128 vector registers (four waves per SIMD) or 106 scalar ones;
* the static LDS stays what it was (784 / 848 bytes): with the kernel's dynamic 39 KB four workgroups share a CU's 160 KB."""
import re

import pytest

import kernel_notes


def _kernels():
    found = {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb([01])ELb([01])EEEv", name)
        if t:
            key = (int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))), bool(int(t.group(4))))       # NS, QS, MEM, FILT
            found[key] = figures
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
