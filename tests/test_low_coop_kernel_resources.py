"""What the compiler made of k_search_low_coop (csrc/fpx_qsearch.hpp, option low_wg = 3 with filt_coop = 1 under query_wg = 2: k_search_filt's
rounds and tasks -- eight lanes to a line behind the group's union dead-set bitmap -- with k_search_low's sorted tail for the queries whose
floor is 1 or 2), read from the built code object through tests/kernel_notes.py the way tests/test_next_kernel_resources.py reads
k_search_next: its eight instantiations (8 / 16 columns x QS x MEM; always FILT) exist and no other kernel carries the name; none is above
128 vector + accumulator registers or 106 scalar ones; the static LDS is 848 bytes at most -- with the dynamic 39 KB four workgroups
share a CU's 160 KB --; and none has more scratch than k_search_query<NS, QS, MEM, true> in the same code object.  The bounds are the ones
k_search_filt and k_search_low_filt meet (tests/test_qs_kernel_resources.py).  No GPU needed.  Fails without the kernel: no such names."""
import re

import pytest

import kernel_notes

QS_LDS_BYTES = (8192 + 4) * 4 + (2 << 11) + (8 << 8) + 32 * 8      # csrc/fpx_qsearch.hpp: records + sink | filter | table | SB_CAND candidates


@pytest.fixture(scope="module")
def built():
    """({(NS, QS, MEM): k_search_low_coop's figures}, {(NS, QS, MEM): those of k_search_query<NS, QS, MEM, true>}, every k_search_low_coop name)"""
    coop, query, names = {}, {}, []
    for name, figures in kernel_notes.kernels().items():
        if "k_search_low_coop" in name:
            names.append(name)
        t = re.match(r"_ZN3fpx17k_search_low_coopILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            coop[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures          # NS, QS, MEM
        t = re.match(r"_ZN3fpx14k_search_queryILi(\d+)ELb([01])ELb([01])ELb1EEEv", name)
        if t:
            query[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return coop, query, names


EIGHT = sorted((ns, qs, mem) for ns in (8, 16) for qs in (False, True) for mem in (False, True))


def test_exactly_eight_instantiations(built):
    coop, query, names = built
    assert sorted(coop) == EIGHT, sorted(coop)
    assert len(names) == 8, names
    assert sorted(query) == EIGHT, sorted(query)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(built):
    coop, _, _ = built
    assert len(coop) == 8, sorted(coop)
    for key, r in coop.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)
        assert r["group_segment_fixed_size"] <= 848, (key, r)
        assert 4 * (QS_LDS_BYTES + r["group_segment_fixed_size"]) <= 160 * 1024, (key, r)


def test_no_more_scratch_than_k_search_query(built):
    coop, query, _ = built
    assert len(coop) == 8, sorted(coop)
    for key, r in coop.items():
        print(key, "k_search_low_coop", r["private_segment_fixed_size"], "k_search_query", query[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= query[key]["private_segment_fixed_size"], (key, r, query[key])
