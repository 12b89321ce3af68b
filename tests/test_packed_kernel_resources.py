"""What the compiler made of k_search_packed (csrc/fpx_qsearch.hpp, option shard_pack: k_search_window's walk with the window's probes
packed before the rounds), read from the built code object the way tests/test_window_kernel_resources.py reads k_search_window's: its
eight instantiations (8 / 16 columns x MEM x FILT) exist and no other kernel carries the name; none is above 128 vector + accumulator
registers or 106 scalar ones; none has more scratch than k_search_window of the same (NS, MEM, FILT) in the same code object -- and the
unfiltered ones have none at all --; and the static LDS is k_search_window's 784 bytes unfiltered and 848 filtered (the packed probes'
count lives in a shared word the window's walk leaves idle, their list where the hash set was), so that with the dynamic 39 KB four
workgroups share a CU's 160 KB.  No GPU needed."""
import re

import pytest

import kernel_notes

QS_LDS_BYTES = (8192 + 4) * 4 + (2 << 11) + (8 << 8) + 32 * 8      # csrc/fpx_qsearch.hpp: records + sink | filter | table | SB_CAND candidates


@pytest.fixture(scope="module")
def built():
    """({(NS, MEM, FILT): k_search_packed's figures}, {(NS, MEM, FILT): k_search_window's}, every name with k_search_packed in it)"""
    packed, win, names = {}, {}, []
    for name, figures in kernel_notes.kernels().items():
        if "k_search_packed" in name:
            names.append(name)
        t = re.match(r"_ZN3fpx15k_search_packedILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            packed[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures          # NS, MEM, FILT
        t = re.match(r"_ZN3fpx15k_search_windowILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            win[(int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))] = figures
    return packed, win, names


EIGHT = sorted((ns, mem, filt) for ns in (8, 16) for mem in (False, True) for filt in (False, True))


def test_exactly_eight_instantiations(built):
    packed, win, names = built
    assert sorted(packed) == EIGHT, sorted(packed)
    assert len(names) == 8, names
    assert sorted(win) == EIGHT, sorted(win)


def test_registers_stay_within_four_waves_per_simd(built):
    packed, _, _ = built
    assert len(packed) == 8, sorted(packed)
    for key, r in packed.items():
        print(key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert r["sgpr_count"] <= 106, (key, r)


def test_no_more_scratch_than_k_search_window(built):
    packed, win, _ = built
    assert len(packed) == 8, sorted(packed)
    for key, r in packed.items():
        print(key, "k_search_packed", r["private_segment_fixed_size"], "k_search_window", win[key]["private_segment_fixed_size"])
        assert r["private_segment_fixed_size"] <= win[key]["private_segment_fixed_size"], (key, r, win[key])
        if not key[2]:
            assert r["private_segment_fixed_size"] == 0, (key, r)


def test_static_lds_keeps_four_workgroups_on_a_cu(built):
    packed, win, _ = built
    assert len(packed) == 8, sorted(packed)
    for key, r in packed.items():
        static = r["group_segment_fixed_size"]
        print(key, "static LDS", static, "k_search_window", win[key]["group_segment_fixed_size"])
        assert 4 * (QS_LDS_BYTES + static) <= 160 * 1024, (key, static)
        assert static <= (848 if key[2] else 784), (key, r)
