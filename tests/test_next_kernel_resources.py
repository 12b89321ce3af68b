"""What the compiler made of k_search_next (csrc/fpx_qsearch.hpp, option groups_wg = 1: k_search_query's walk over a group that is not the
first of its batch's, the hand-over chained behind the launch before), read from the built code object the way
tests/test_qs_kernel_resources.py reads the other kernels of the family: its eight instantiations (8 / 16 columns x QS x FILT; never MEM)
exist and no other; none is above 128 vector registers or 106 scalar ones; the static LDS is 784 bytes at most unfiltered and 848
filtered -- with the dynamic 39 KB four workgroups share a CU --; and none has more scratch than k_search_query<NS, QS, false, FILT> in the
same code object.  No GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def built():
    """({(NS, QS, FILT): k_search_next's figures}, {(NS, QS, FILT): those of k_search_query<NS, QS, false, FILT>}, every k_search_next name)"""
    nxt, query, names = {}, {}, []
    for name, figures in kernel_notes.kernels().items():
        if "k_search_next" in name:
            names.append(name)
        t = re.match(r"_ZN3fpx13k_search_nextILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            nxt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures           # NS, QS, FILT
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb0ELb([01])EEEv", name)
        if t:
            query[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return nxt, query, names


EIGHT = sorted((ns, qs, filt) for ns in (8, 16) for qs in (False, True) for filt in (False, True))


def test_exactly_eight_instantiations(built):
    nxt, query, names = built
    assert sorted(nxt) == EIGHT, sorted(nxt)
    assert len(names) == 8, names
    assert sorted(query) == EIGHT, sorted(query)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    nxt, _, _ = built
    assert len(nxt) == 8, sorted(nxt)
    for key, r in nxt.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= (848 if key[2] else 784), (key, r)


def test_no_more_scratch_than_k_search_query(built):
    nxt, query, _ = built
    assert len(nxt) == 8, sorted(nxt)
    for key, r in nxt.items():
        print(key, "k_search_next", r["private_segment_fixed_size"], "k_search_query", query[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= query[key]["private_segment_fixed_size"], (key, r, query[key])
