"""What the compiler made of k_search_filt (csrc/fpx_qsearch.hpp, option filt_coop = 1 under query_wg = 2: the filtered walk eight lanes
to a line, behind the group's union dead-set bitmap), read from the built code object the way tests/test_low_filt_kernel_resources.py
reads k_search_low_filt's: its eight instantiations (8 / 16 columns x QS x MEM) exist; none is above 128 vector registers or 106 scalar
ones, and the static LDS is the filtered form's 848 bytes at most -- with the dynamic 39 KB four workgroups share a CU --; and none has
more scratch than k_search_query's FILTERED instantiation of the same (NS, QS, MEM) in the same code object.  No GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def built():
    """({(NS, QS, MEM): k_search_filt's figures}, {(NS, QS, MEM): those of k_search_query<NS, QS, MEM, true>})"""
    filt, query_filt = {}, {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx13k_search_filtILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            filt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures       # NS, QS, MEM
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb([01])ELb1EEEv", name)
        if t:
            query_filt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return filt, query_filt


EIGHT = sorted((ns, qs, mem) for ns in (8, 16) for qs in (False, True) for mem in (False, True))


def test_eight_instantiations(built):
    filt, query_filt = built
    assert sorted(filt) == EIGHT, sorted(filt)
    assert sorted(query_filt) == EIGHT, sorted(query_filt)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    filt, _ = built
    assert len(filt) == 8, sorted(filt)
    for key, r in filt.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= 848, (key, r)


def test_no_more_scratch_than_the_filtered_k_search_query(built):
    filt, query_filt = built
    assert len(filt) == 8, sorted(filt)
    for key, r in filt.items():
        print(key, "k_search_filt", r["private_segment_fixed_size"], "k_search_query filtered", query_filt[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= query_filt[key]["private_segment_fixed_size"], (key, r, query_filt[key])
