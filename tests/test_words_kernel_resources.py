"""What the compiler made of k_search_words (csrc/fpx_qwords.hpp), read from the built code object the way tests/test_qs_kernel_resources.py
reads k_search_query's: its eight instantiations (8 / 16 columns x MEM x FILT) exist, none is above 128 vector registers (four workgroups
per CU next to 39 KB of dynamic LDS each), the unfiltered ones have no scratch segment and spill no vector register, and the static LDS
leaves room for four workgroups in a CU's 160 KB -- no GPU needed."""
import re

import pytest

import kernel_notes

WORDS_LDS_BYTES = (8192 + 4) * 4 + (2 << 11) + (8 << 8) + 32 * 8       # SIDE_LDS_BYTES: records, filter, exact table, candidate buffer (SB_CAND = 32)


@pytest.fixture(scope="module")
def words():
    found = {}
    for name, figures in kernel_notes.kernels().items():
        t = re.match(r"_ZN3fpx14k_search_wordsILi(\d+)ELb([01])ELb([01])EEEv", name)
        if t:
            key = (int(t.group(1)), bool(int(t.group(2))), bool(int(t.group(3))))       # NS, MEM, FILT
            found[key] = figures
    return found


def test_eight_instantiations(words):
    assert sorted(words) == sorted((ns, mem, filt) for ns in (8, 16) for mem in (False, True) for filt in (False, True)), sorted(words)


def test_registers_and_lds_keep_four_workgroups_on_a_cu(words):
    assert len(words) == 8, sorted(words)
    for key, r in words.items():
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (key, r)
        assert 4 * (r["group_segment_fixed_size"] + WORDS_LDS_BYTES) <= 160 * 1024, (key, r)


def test_unfiltered_kernels_have_no_scratch_and_no_vector_spills(words):
    assert len(words) == 8, sorted(words)
    for key, r in words.items():
        if not key[2]:
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (key, r)
