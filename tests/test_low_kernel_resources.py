"""What the compiler made of k_search_low (csrc/fpx_qsearch.hpp, option low_wg), read from the built code object the way
tests/test_kernel_resources.py reads k_search_query's: its eight instantiations (8 / 16 columns x QS x MEM) exist, none has a scratch
segment or spills a vector register, none is above 128 vector registers or 106 scalar ones, and the static LDS is k_search_query's 784
bytes (the sorted tail's scratch is the filter's area): with the dynamic 39 KB four workgroups share a CU -- no GPU needed."""
import glob
import os
import re

import pytest

from test_kernel_resources import FIELDS, PKG, _notes      # (the same reader)


@pytest.fixture(scope="module")
def low():
    lib = os.path.join(PKG, "libfpx.so")
    search_o = os.path.join(PKG, "build", "fpx_search.o")
    if not glob.glob(os.path.join(PKG, "build", "*.o")) and not os.path.exists(lib):
        pytest.skip("nothing built: neither libfpx.so nor build/*.o")
    notes = _notes(lib if os.path.exists(lib) else search_o)
    found = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n\s+- \.agpr_count:|\namdhsa\.target|\Z)", notes, flags=re.S):
        blk = m.group(0)
        t = re.search(r"\.name:\s+_ZN3fpx12k_search_lowILi(\d+)ELb([01])ELb([01])EEEv", blk)
        if t:
            key = (int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))       # NS, QS, MEM
            found[key] = {f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1)) for f in FIELDS}
    return found


def test_eight_instantiations(low):
    assert sorted(low) == sorted((ns, qs, mem) for ns in (8, 16) for qs in (False, True) for mem in (False, True)), sorted(low)


def test_no_scratch_and_no_vector_spills(low):
    assert len(low) == 8, sorted(low)
    for key, r in low.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (key, r)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(low):
    assert len(low) == 8, sorted(low)
    for key, r in low.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= 784, (key, r)
