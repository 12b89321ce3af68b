"""What the compiler made of k_search_low (csrc/fpx_qsearch.hpp, option low_wg), read from the built code object the way
tests/test_kernel_resources.py reads k_search_query's: its eight instantiations (8 / 16 columns x QS x MEM) exist, none has a scratch
segment or spills a vector register, none is above 128 vector registers or 106 scalar ones, and the static LDS is k_search_query's 784
bytes (the sorted tail's scratch is the filter's area): with the dynamic 39 KB four workgroups share a CU -- no GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def low():
    found = {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx12k_search_lowILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            key = (int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))       # NS, QS, MEM
            found[key] = figures
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
