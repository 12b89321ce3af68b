"""What the compiler made of k_search_classes (csrc/fpx_qsearch.hpp), read from the built code object the way tests/test_kernel_resources.py
reads k_search_query's: its four instantiations (8 / 16 columns x MEM) exist, none has a scratch segment or spills a vector register, and
none is above 128 vector registers (the occupancy k_search_query's body was written for) -- no GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def classes():
    found = {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx16k_search_classesILi(\d+)ELb([01])EEEv", name)
        if t:
            found[(int(t.group(1)), bool(int(t.group(2))))] = figures      # NS, MEM
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
