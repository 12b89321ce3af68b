"""What the compiler made of k_search_window (csrc/fpx_qsearch.hpp, option shard_wg: k_search_query's walk over a rank's hash-window slice
of a packed group, the query's records copied into its bin of the sharded protocol's send buffer), read from the built code object the
way tests/test_next_kernel_resources.py reads k_search_next's: its eight instantiations (8 / 16 columns x MEM x FILT; never QS) exist and
no other; none is above 128 vector registers or 106 scalar ones; the static LDS is 784 bytes at most unfiltered and 848 filtered -- with
the dynamic 39 KB four workgroups share a CU --; and none has more scratch than k_search_query<NS, false, MEM, FILT> in the same code
object.  No GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def built():
    """({(NS, MEM, FILT): k_search_window's figures}, {(NS, MEM, FILT): those of k_search_query<NS, false, MEM, FILT>}, every k_search_window name)"""
    win, query, names = {}, {}, []
    for name, figures in kernel_notes.kernels().items():
        if "k_search_window" in name:
            names.append(name)
        t = re.match(r"_ZN3fpx15k_search_windowILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            win[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures             # NS, MEM, FILT
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb0ELb([01])ELb([01])EEEv", name)
        if t:
            query[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return win, query, names


EIGHT = sorted((ns, mem, filt) for ns in (8, 16) for mem in (False, True) for filt in (False, True))


def test_exactly_eight_instantiations(built):
    win, query, names = built
    assert sorted(win) == EIGHT, sorted(win)
    assert len(names) == 8, names
    assert sorted(query) == EIGHT, sorted(query)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    win, _, _ = built
    assert len(win) == 8, sorted(win)
    for key, r in win.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= (848 if key[2] else 784), (key, r)


def test_no_more_scratch_than_k_search_query(built):
    win, query, _ = built
    assert len(win) == 8, sorted(win)
    for key, r in win.items():
        print(key, "k_search_window", r["private_segment_fixed_size"], "k_search_query", query[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= query[key]["private_segment_fixed_size"], (key, r, query[key])
