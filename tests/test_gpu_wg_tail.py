"""The tail that k_search_side and k_search_words share (csrc/fpx_qframe.hpp: filter counting, the exact table with its passes, the candidate
buffer, the hand-over) AT its thresholds, which the crowded-query tests of test_gpu_side_wg.py and test_gpu_words_wg.py jump over: they go
straight to 200 and more candidates.  N docs of one segment / column share five hashes, a query holds those five and sixty random ones,
the floor is 5: exactly N candidates, for

    N =   4 |   5   the query's QCAND_SLOTS own slots | the shared list (from 5 to 32: through the hand-over alone, s_cshared still 0)
    N =  32 |  33   the SB_CAND entries of the LDS buffer | the buffer overflowing into the list
    N = 192 | 193   three quarters of the exact table | the passes doubled
    N = 300         more than the table takes: the passes really iterate

all as queries of ONE batch, with aimed queries between them -- a batch of more queries than the chip holds workgroups (four per CU), in
cycles of nine, so that a workgroup takes several queries and meets a different N each time: what one query leaves in the workgroup's
state the next one finds.  The worlds are wg_harness.py's, with the two files' settings."""
import numpy as np
import pytest

import wg_harness as wg
from wg_harness import U64, WORDS_LO, WORDS_HI, aimed, figures as _figures, rand_items

pytestmark = pytest.mark.gpu

NS = (4, 5, 32, 33, 192, 193, 300)
KERNELS = {"side": ("side_wg", wg.SIDE), "words": ("words_wg", wg.WORDS)}      # the option, the kernel's bit of fpx_stats.path_flags
SECOND_TRIP = wg.SECOND_TRIP
BATCH, CYCLE = 1200, 9                # (CYCLE: the seven N and two aimed queries; 9 divides no grid of 4 x a power of two)
SEED = 1600                           # (with it the oracle alone gives every N-doc query exactly N results: checked before this was committed)
OPTIONS = ("words_wg", "side_wg", "query_wg", "direct_min_items")


def _five(n):
    """the five hashes that N docs share (inside every column's hash range)"""
    return np.array([0x51515151 + (n * 8 + k) * 7919 for k in range(5)], dtype=np.uint32)


def _shared_rows(ids):
    """for every N: N docs of `ids` -- the ranges apart -- under its five hashes"""
    rows, at = [], 0
    for n in NS:
        rows += [(int(h), ids[at: at + n]) for h in _five(n)]
        at += n
    return rows


def side_world(Pair, ctx, rng):
    """a young index: two checkpoints in blocks (small decoded), one segment direct-addressed alone; the shared hashes in the first"""
    w = wg.World(Pair, ctx, packed=1, form="blocks")
    ids = np.arange(1, 1501)
    w.file(rand_items(rng, ids, 40, _shared_rows(ids)), ids)
    w.file(rand_items(rng, np.arange(1501, 2501), 40), np.arange(1501, 2501))
    w.file(rand_items(rng, np.arange(2501, 4001), 40), np.arange(2501, 4001), form="alone")
    return w, w.finish()


def words_world(Pair, ctx, rng):
    """one group of four columns in directory + words form; the shared hashes in column 0"""
    w = wg.World(Pair, ctx, packed=0, lo=WORDS_LO, hi=WORDS_HI)
    p, _ = w.columns(rng, 4, 1200, 40, lambda s, ids: _shared_rows(ids) if s == 0 else [])
    return w, p


def make_queries(rng, items):
    """BATCH queries in cycles of nine: the seven N-doc queries and two aimed ones, every other cycle aimed ones only (the batch's
    candidates stay below the shared list's first size, 64 per query: more would hand the batch back).  -> the queries, {position: N}"""
    of_n = {}
    for n in NS:
        q = np.concatenate([_five(n), rng.integers(0, 1 << 32, 60, dtype=U64).astype(np.uint32)])
        rng.shuffle(q)
        of_n[n] = q
    queries, where = [], {}
    for i in range(BATCH):
        if i % CYCLE < len(NS) and (i // CYCLE) % 2 == 0:
            where[i] = NS[i % CYCLE]
            queries.append(of_n[where[i]])
        else:
            queries.append(aimed(rng, items[i % len(items)], 65))
    return queries, where


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_tail_at_its_thresholds(env, monkeypatch, kernel):
    fpx, oracle, Pair, ctx = env
    option, bit = KERNELS[kernel]
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    wg.reset(ctx, OPTIONS)
    ctx.set_option("group_packed", 1 if kernel == "side" else 0)
    rng = np.random.default_rng(SEED)
    try:
        w, p = (side_world if kernel == "side" else words_world)(Pair, ctx, rng)
        queries, where = make_queries(rng, w.items)
        opts = fpx.SearchOptions(max_results=max(NS), min_score=5, min_score_pct=0)
        four = next(i for i, n in where.items() if n == 4)
        assert sum(where.values()) < 1 << 16 and set(where.values()) == set(NS)  # (the shared list takes the batch's candidates: nothing is handed back)
        ctx.set_option(option, 1)
        got, st = p.check(queries, opts)                                       # (results and scanned blocks / docs == the oracle's, per query)
        got_four, st_four = p.reader.search_batch([queries[four]] * 2, opts)   # (the N = 4 query alone; a batch of ONE is the pipeline's)
        ctx.set_option(option, 0)
        got0, st0 = p.reader.search_batch(queries, opts)
    finally:
        wg.reset(ctx, OPTIONS)
    print(f"{kernel}: {option} 1: path_flags {st.path_flags}, {_figures(st)}; 0: {st0.path_flags}, {_figures(st0)}; N = 4 alone: {st_four.path_flags}")
    assert st.path_flags & bit and st.path_flags & SECOND_TRIP, st.path_flags
    assert not st0.path_flags & bit, st0.path_flags
    assert got == got0
    assert _figures(st) == _figures(st0), (_figures(st), _figures(st0))
    assert st_four.path_flags & bit and not st_four.path_flags & SECOND_TRIP, st_four.path_flags
    assert got_four == [got[four]] * 2
    for i, n in where.items():
        assert len(got[i]) == n and all(score == 5 for _, score in got[i]), (i, n, len(got[i]))
    assert all(got[i] and got[i][0][1] >= 5 for i in range(BATCH) if i not in where)
