"""What the compiler made of the query-per-workgroup family of csrc/fpx_qsearch.hpp -- the nine kernels over qs_body --, read from the
built gfx950 code objects through tests/kernel_notes.py the way tools/kernel_resources.py reads them.  ONE table, a row per kernel; every
test is parametrised by kernel, so a failure names it.  No GPU needed.  (k_search_next, k_search_low_next, k_search_window and
k_search_packed still have a file each, test_<name>_kernel_resources.py, with the same assertions.)

* instantiations: exactly the kernel's template parameters' combinations exist (`unique`: and no other kernel carries the name); where a
  row compares against another kernel, that kernel's counterparts are all there too;
* registers: at most 128 vector + accumulator registers (four waves per SIMD) and, where the row says so, 106 scalar ones;
* static LDS: at most 784 bytes unfiltered, 848 filtered -- with the dynamic 39 KB four workgroups share a CU's 160 KB;
* scratch: none at all (and no vector register spilled), or no more than the kernel it was made from in the same code object --
  k_search_query's filtered instantiations themselves are bounded at what they had when the unfiltered ones lost theirs: 88 bytes at 16
  columns, 24 at 8."""
import collections
import itertools
import re

import pytest

import kernel_notes

QS_LDS_BYTES = (8192 + 4) * 4 + (2 << 11) + (8 << 8) + 32 * 8      # csrc/fpx_qsearch.hpp: records + sink | filter | table | SB_CAND candidates

# params: the kernel's template parameters, in order (NS: 8 | 16, the others bool); fixed: what the kernel's form settles of the others;
# sgpr, lds: the row bounds them; scratch: "none" | "none unfiltered" (k_search_query: and the filtered ones at 88 / 24 bytes) | "";
# than: no more scratch than this kernel's instantiation of the same values
Row = collections.namedtuple("Row", "params fixed sgpr lds unique scratch than")
TABLE = {
    "k_search_query":    Row(("NS", "QS", "MEM", "FILT"), {},                             True,  True,  False, "none unfiltered", None),
    "k_search_classes":  Row(("NS", "MEM"),               {"QS": True, "FILT": False},    False, False, False, "none",            None),
    "k_search_low":      Row(("NS", "QS", "MEM"),         {"FILT": False},                True,  True,  False, "none",            None),
    "k_search_low_filt": Row(("NS", "QS", "MEM"),         {"FILT": True},                 True,  True,  False, "",                "k_search_query"),
    "k_search_filt":     Row(("NS", "QS", "MEM"),         {"FILT": True},                 True,  True,  False, "",                "k_search_query"),
    "k_search_next":     Row(("NS", "QS", "FILT"),        {"MEM": False},                 True,  True,  True,  "",                "k_search_query"),
    "k_search_low_next": Row(("NS", "QS", "FILT"),        {"MEM": False},                 True,  True,  True,  "",                "k_search_next"),
    "k_search_window":   Row(("NS", "MEM", "FILT"),       {"QS": False},                  True,  True,  True,  "",                "k_search_query"),
    "k_search_packed":   Row(("NS", "MEM", "FILT"),       {"QS": False},                  True,  True,  True,  "none unfiltered", "k_search_window"),
}


def _combinations(params):
    return sorted(itertools.product(*[(8, 16) if p == "NS" else (False, True) for p in params]))


@pytest.fixture(scope="module")
def built():
    """{kernel: ({its parameters' values: figures}, every built name that contains the kernel's name)}"""
    out = {}
    for kernel, row in TABLE.items():
        rx = re.compile(r"_ZN3fpx%d%sI%sEEv" % (len(kernel), kernel, "".join(r"Li(\d+)E" if p == "NS" else "Lb([01])E" for p in row.params)))
        found, names = {}, []
        for name, figures in kernel_notes.kernels().items():
            if kernel in name:
                names.append(name)
            t = rx.match(name)
            if t:
                found[tuple(int(v) if p == "NS" else bool(int(v)) for p, v in zip(row.params, t.groups()))] = figures
        out[kernel] = (found, names)
    return out


def _complete(built, kernel):
    found, _ = built[kernel]
    assert sorted(found) == _combinations(TABLE[kernel].params), (kernel, sorted(found))
    return found


def _values(kernel, key):
    return dict(TABLE[kernel].fixed, **dict(zip(TABLE[kernel].params, key)))


def _counterpart(built, kernel, key):
    """the figures of TABLE[kernel].than for the same values"""
    than, v = TABLE[kernel].than, _values(kernel, key)
    return built[than][0][tuple(v[p] for p in TABLE[than].params)]


@pytest.mark.parametrize("kernel", TABLE)
def test_exactly_its_instantiations(built, kernel):
    row = TABLE[kernel]
    found = _complete(built, kernel)
    if row.unique:
        assert len(built[kernel][1]) == len(found), built[kernel][1]
    if row.than:
        _complete(built, row.than)
        for key in found:
            _counterpart(built, kernel, key)


@pytest.mark.parametrize("kernel", TABLE)
def test_registers_and_lds_keep_four_workgroups_on_a_cu(built, kernel):
    row = TABLE[kernel]
    for key, r in _complete(built, kernel).items():
        print(kernel, key, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (kernel, key, r)
        if row.sgpr:
            assert r["sgpr_count"] <= 106, (kernel, key, r)
        if row.lds:
            static = r["group_segment_fixed_size"]
            assert static <= (848 if _values(kernel, key)["FILT"] else 784), (kernel, key, r)
            assert 4 * (QS_LDS_BYTES + static) <= 160 * 1024, (kernel, key, static)


@pytest.mark.parametrize("kernel", TABLE)
def test_scratch(built, kernel):
    row = TABLE[kernel]
    for key, r in _complete(built, kernel).items():
        v, scratch = _values(kernel, key), r["private_segment_fixed_size"]
        if row.scratch == "none" or (row.scratch == "none unfiltered" and not v["FILT"]):
            assert scratch == 0 and r["vgpr_spill_count"] == 0, (kernel, key, r)
        elif kernel == "k_search_query":
            assert scratch <= (88 if v["NS"] == 16 else 24), (kernel, key, r)
        if row.than:
            other = _counterpart(built, kernel, key)
            print(kernel, key, scratch, row.than, other["private_segment_fixed_size"])
            assert scratch <= other["private_segment_fixed_size"], (kernel, key, r, other)
