"""What the compiler made of k_search_classes (csrc/fpx_qsearch.hpp), read from the built code object the way tests/test_kernel_resources.py
reads k_search_query's: its four instantiations (8 / 16 columns x MEM) exist, none has a scratch segment or spills a vector register, and
none is above 128 vector registers (the occupancy k_search_query's body was written for) -- no GPU needed."""
import glob
import os
import re

import pytest

from test_kernel_resources import FIELDS, PKG, _notes      # (the same reader)


@pytest.fixture(scope="module")
def classes():
    lib = os.path.join(PKG, "libfpx.so")
    search_o = os.path.join(PKG, "build", "fpx_search.o")
    if not glob.glob(os.path.join(PKG, "build", "*.o")) and not os.path.exists(lib):
        pytest.skip("nothing built: neither libfpx.so nor build/*.o")
    notes = _notes(lib if os.path.exists(lib) else search_o)
    found = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n\s+- \.agpr_count:|\namdhsa\.target|\Z)", notes, flags=re.S):
        blk = m.group(0)
        t = re.search(r"\.name:\s+_ZN3fpx16k_search_classesILi(\d+)ELb([01])EEEv", blk)
        if t:
            found[(int(t.group(1)), bool(int(t.group(2))))] = {f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1)) for f in FIELDS}      # NS, MEM
    return found


def test_four_instantiations(classes):
    assert sorted(classes) == sorted((ns, mem) for ns in (8, 16) for mem in (False, True)), sorted(classes)


def test_no_scratch_and_no_vector_spills(classes):
    assert len(classes) == 4, sorted(classes)
    for key, r in classes.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (key, r)


def test_registers(classes):
    assert len(classes) == 4, sorted(classes)
    for key, r in classes.items():
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
