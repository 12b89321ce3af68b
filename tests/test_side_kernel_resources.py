"""What the compiler made of k_search_side (csrc/fpx_qside.hpp), read from the built code object the way tests/test_qs_kernel_resources.py
reads k_search_query's: the kernel exists, has no scratch segment and spills no vector register, and its registers and static LDS leave
room for four workgroups on a CU next to the 39 KB of dynamic LDS it is launched with -- no GPU needed."""
import re

import pytest

import kernel_notes


@pytest.fixture(scope="module")
def side():
    found = []
    for name, figures in kernel_notes.kernels().items():
        if re.match(r"_ZN3fpx13k_search_sideE", name):
            found.append(figures)
    assert len(found) == 1, f"k_search_side: {len(found)} kernels of that name in the built code object, one expected"
    return found[0]


def test_no_scratch_and_no_vector_spills(side):
    assert side["private_segment_fixed_size"] == 0 and side["vgpr_spill_count"] == 0, side


def test_registers_and_lds_keep_four_workgroups_on_a_cu(side):
    assert side["vgpr_count"] + side["agpr_count"] <= 128, side           # four waves per SIMD: a workgroup is a wave on each
    assert side["group_segment_fixed_size"] <= 1024, side                 # + 39 KB dynamic: four workgroups share a CU's 160 KB
