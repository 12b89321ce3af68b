"""What the compiler made of k_search_low_next (csrc/fpx_qsearch.hpp, option groups_wg = 2 with low_wg: k_search_next's walk over a group
that is not the first of its batch's, with k_search_low's sorted tail for the queries whose floor is 1 or 2 and the chained hand-over
behind either tail), read from the built code object the way tests/test_next_kernel_resources.py reads k_search_next's: its eight
instantiations (8 / 16 columns x QS x FILT; never MEM) exist and no other; none is above 128 vector registers or 106 scalar ones; the
static LDS is 784 bytes at most unfiltered and 848 filtered -- with the dynamic 39 KB four workgroups share a CU --; and none has more
scratch than k_search_next<NS, QS, FILT> in the same code object.  No GPU needed.  On a tree without the kernel the first two tests
fail (no instantiation is found)."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def built():
    """({(NS, QS, FILT): k_search_low_next's figures}, {(NS, QS, FILT): those of k_search_next<NS, QS, FILT>}, every k_search_low_next name)"""
    low_next, nxt, names = {}, {}, []
    for name, figures in kernel_notes.kernels().items():
        if "k_search_low_next" in name:
            names.append(name)
        t = re.match(r"_ZN3fpx17k_search_low_nextILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            low_next[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures       # NS, QS, FILT
        t = re.match(r"_ZN3fpx13k_search_nextILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            nxt[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return low_next, nxt, names


EIGHT = sorted((ns, qs, filt) for ns in (8, 16) for qs in (False, True) for filt in (False, True))


def test_exactly_eight_instantiations(built):
    low_next, nxt, names = built
    assert sorted(low_next) == EIGHT, sorted(low_next)
    assert len(names) == 8, names
    assert sorted(nxt) == EIGHT, sorted(nxt)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    low_next, _, _ = built
    assert len(low_next) == 8, sorted(low_next)
    for key, r in low_next.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= (848 if key[2] else 784), (key, r)


def test_no_more_scratch_than_k_search_next(built):
    low_next, nxt, _ = built
    assert len(low_next) == 8, sorted(low_next)
    for key, r in low_next.items():
        print(key, "k_search_low_next", r["private_segment_fixed_size"], "k_search_next", nxt[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= nxt[key]["private_segment_fixed_size"], (key, r, nxt[key])
