"""What the compiler made of k_search_low_filt (csrc/fpx_qsearch.hpp, option low_wg = 2 under query_wg = 2: the filtered walk with the
sorted tail), read from the built code object the way tests/test_kernel_resources.py reads k_search_query's: its eight instantiations
(8 / 16 columns x QS x MEM) exist; none is above 128 vector registers or 106 scalar ones, and the static LDS is the filtered form's 848
bytes at most -- with the dynamic 39 KB four workgroups share a CU --; and none has more scratch than k_search_query's FILTERED
instantiation of the same (NS, QS, MEM) in the same code object, which tests/test_kernel_resources.py bounds at 88 / 24 bytes.  No GPU
needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def built():
    """({(NS, QS, MEM): k_search_low_filt's figures}, {(NS, QS, MEM): those of k_search_query<NS, QS, MEM, true>})"""
    low_filt, query_filt = {}, {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx17k_search_low_filtILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            low_filt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures       # NS, QS, MEM
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb([01])ELb1EEEv", name)
        if t:
            query_filt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return low_filt, query_filt


EIGHT = sorted((ns, qs, mem) for ns in (8, 16) for qs in (False, True) for mem in (False, True))


def test_eight_instantiations(built):
    low_filt, query_filt = built
    assert sorted(low_filt) == EIGHT, sorted(low_filt)
    assert sorted(query_filt) == EIGHT, sorted(query_filt)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    low_filt, _ = built
    assert len(low_filt) == 8, sorted(low_filt)
    for key, r in low_filt.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= 848, (key, r)


def test_no_more_scratch_than_the_filtered_k_search_query(built):
    low_filt, query_filt = built
    assert len(low_filt) == 8, sorted(low_filt)
    for key, r in low_filt.items():
        print(key, "k_search_low_filt", r["private_segment_fixed_size"], "k_search_query filtered", query_filt[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= query_filt[key]["private_segment_fixed_size"], (key, r, query_filt[key])
