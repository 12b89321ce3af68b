"""Option shard_pack (csrc/fpx_qsearch.hpp: k_search_packed; csrc/fpx_search.hip: shard_probe_impl): a step of the sharded bin protocol
that option shard_wg lets walk its window a query per workgroup packs the window's first occurrences BEFORE the rounds -- a hash outside
the window never enters the dedup set, the probes get dense places 0 .. m - 1, the rounds are ceil(m / 256) and a wave without a probe
skips its round -- where the batch's longest query has at most 1024 hashes.  The bins are the protocol's as they were: every case
compares the step under (shard_wg 2, shard_pack 1) against the step under shard_wg 0 with tests/test_gpu_shard_wg.py's _compare (every
bin's records, nulls dropped and sorted, and the width bit; blocks, docs, probes and hits summed over the ranks against the unsharded
batch's; the results after fpx_shard_score against the unsharded snapshot's and the oracle's, query by query), asserts
fpx_stats.path_flags bit 15 (with 14, 6 and 4) on every rank that should have packed and its absence under 0, and a non-zero record
total on the rank under test.  The constructed cases assert the docs they planted by id.

The worlds, the fixtures and the steps are test_gpu_shard_wg.py's (3 segments x 5000 docs x 64 hashes, packed, one world at a time).

On a library without the feature the option's name is refused: every case fails at its first set_option."""
import contextlib
import functools

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import HOT1, HOT8
from test_gpu_shard_wg import (DEDUP_MAX, EDGES, H, ONES, PATTERN, PER, QUERY_WG, S, WALKED, Ranks, Step, _compare, _equal_cells, _Kept, _made,
                               _queries, _three, _world_data, env, kept_world_goes_with_the_module, tidy)      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

PACKED = 1 << 15
ALL_FOUR = PACKED | WALKED | QUERY_WG | 16
FPX_E_INVAL = -4                                     # include/fpx.h
PACK_MAX = 1024                                      # csrc/fpx_qsearch.hpp: QS_PACK_MAX, the longest query k_search_packed takes
U64 = np.uint64


@pytest.fixture(autouse=True)
def pack_goes_back(env, tidy):
    """shard_pack at its fallback before and after every case (tidy does the same for shard_wg and the storage options)"""
    ctx = env[3]
    ctx.set_option("shard_pack", -1)
    try:
        yield
    finally:
        ctx.set_option("shard_pack", -1)


@contextlib.contextmanager
def packing(ctx, value=1):
    ctx.set_option("shard_pack", value)
    try:
        yield
    finally:
        ctx.set_option("shard_pack", -1)


def _records(step, r):
    return sum(len(recs) for recs, _ in step.cells()[r])


def _check_flags(on, off, packed, rank):
    want = [packed] * on.w.world if isinstance(packed, bool) else list(packed)
    assert [(f & PACKED) != 0 for f in on.flags()] == want, (on.flags(), want)
    assert all(f & ALL_FOUR == ALL_FOUR for f, x in zip(on.flags(), want) if x), on.flags()
    assert not any(f & PACKED for f in off.flags()), off.flags()
    assert _records(on, rank) > 0, "the rank under test stored no record: the case compares nothing"


def _pcompare(w, queries, opts, level=2, packed=True, walked=True, cell_cap=16, rank=0):
    """_compare under shard_pack 1 (the step under `level` against the step under 0), then bit 15: on every rank (or one flag per rank in
    `packed`) together with 14, 6 and 4, clear under 0; and records on `rank`"""
    with packing(w.ctx):
        on, off = _compare(w, queries, opts, level, walked=walked, cell_cap=cell_cap)
    _check_flags(on, off, packed, rank)
    return on, off


def _ids(result):
    return [d for d, _ in result]


# ---- what a constructed query is made of -----------------------------------------------------------------------------------------

class Pool:
    """the hashes of the kept world's postings inside [lo, hi], by how many postings each has (dead ones counted: an upper bound of
    the records): `rare` -- at most two postings, what a query is filled with --, and own(doc): a doc's hashes there with at most 50"""

    def __init__(self, fpx, world, lo, hi, data=None):
        self.lo, self.hi = lo, hi
        self.data = _world_data(fpx, np.random.default_rng(world), edges=True) if data is None else data     # (_Kept.get's bytes: the same seed)
        h = np.concatenate([(items >> U64(32)).astype(np.uint32) for items, *_ in self.data])
        self.u, self.c = np.unique(h[(h >= lo) & (h <= hi)], return_counts=True)
        self.rare = self.u[self.c <= 2]

    def own(self, doc, most=16):
        """(the last segment's own docs are superseded by nobody)"""
        hs = np.unique(wg.rows(self.data[-1][0], doc))
        hs = hs[(hs >= self.lo) & (hs <= self.hi)]
        hs = hs[self.c[np.searchsorted(self.u, hs)] <= 50]
        return hs[:most]

    def outside(self, rng, k):
        out = np.zeros(0, np.uint32)
        while len(out) < k:
            v = wg.noise(rng, 2 * k + 8)
            out = np.concatenate([out, v[(v < self.lo) | (v > self.hi)]])
        return out[:k]

    def inside(self, rng, doc, m):
        """m distinct hashes of the window: the doc's own first, rare ones of the world beyond"""
        own = self.own(doc)[:m]
        rest = rng.choice(np.setdiff1d(self.rare, own), m - len(own), replace=False).astype(np.uint32)
        return np.concatenate([own, rest]), len(own)

    def count(self, q):
        return len(np.unique(q[(q >= self.lo) & (q <= self.hi)]))


LAST = 2 * PER                                       # the last segment's own docs: LAST + 1 .. LAST + PER


# ---- the 2-rank world: parity, FPX_E_AGAIN, the option ------------------------------------------------------------------------------

def _parity(env, world):
    w, fpx = _Kept.get(env, world), env[0]
    for opts in _three(fpx):
        _pcompare(w, _queries(fpx), opts, 2, rank=world - 1)


def _parity_unfiltered(env, world):
    fpx = env[0]
    with _made(env, world, _world_data(fpx, np.random.default_rng(world), again=False)) as w:
        for opts in _three(fpx):
            _pcompare(w, _queries(fpx), opts, 1, rank=world - 1)


def test_parity_on_a_filtered_world_at_2_ranks(env):
    _parity(env, 2)


def test_a_bin_over_its_capacity_says_what_it_needs(env):
    """cell_cap = 16 first: the call returns the need, the retry with the ranks' largest succeeds -- the same need under 0 and under the
    packed kernel.  The send buffer holds a pattern before each call: after the succeeding one every cell behind a bin's count still
    holds it, and none below does"""
    w = _Kept.get(env, 2)
    fpx = w.fpx
    qb = fpx.QueryBatch(w.ctx, _queries(fpx), fpx.SearchOptions(500, 3, 10))
    with packing(w.ctx):
        on, off = Step(w, qb, 2, cell_cap=16, fill=PATTERN), Step(w, qb, 0, cell_cap=16, fill=PATTERN)
    for step in (on, off):
        assert step.attempts == 2 and step.cell_cap > 16, (step.attempts, step.cell_cap)
    assert on.cell_cap == off.cell_cap                                # (the same counts: the same need)
    _check_flags(on, off, True, 0)
    for ra, rb in zip(on.cells(fill=PATTERN), off.cells()):
        for (xa, na), (xb, nb) in zip(ra, rb):
            assert na == nb and len(xa) == len(xb) and (xa == xb).all()
    assert on.results() == off.results()
    qb.release()


def test_the_option_round_trips(env, monkeypatch):
    fpx, ctx = env[0], env[3]
    monkeypatch.delenv("FPX_SHARD_PACK", raising=False)
    assert ctx.get_option("shard_pack") == 0                          # the default
    for v in (0, 1):
        ctx.set_option("shard_pack", v)
        assert ctx.get_option("shard_pack") == v
    with pytest.raises(fpx.FpxError) as refused:
        ctx.set_option("shard_pack", 2)
    assert refused.value.status == FPX_E_INVAL and "shard_pack is 0 or 1" in str(refused.value), refused.value
    assert ctx.get_option("shard_pack") == 1                          # a refused value changes nothing
    monkeypatch.setenv("FPX_SHARD_PACK", "1")
    ctx.set_option("shard_pack", 0)
    assert ctx.get_option("shard_pack") == 0
    ctx.set_option("shard_pack", -1)
    assert ctx.get_option("shard_pack") == 1                          # back to the fallback: the environment, read per call
    monkeypatch.delenv("FPX_SHARD_PACK")
    assert ctx.get_option("shard_pack") == 0
    # under shard_wg 0 the option does nothing: the same flags, cells and results with it and without
    w = _Kept.get(env, 2)
    qb = fpx.QueryBatch(w.ctx, _queries(fpx)[:40], fpx.SearchOptions(500, 3, 10))
    with packing(ctx):
        with_it = Step(w, qb, 0)
    without = Step(w, qb, 0)
    assert with_it.flags() == without.flags() and not any(f & (PACKED | WALKED | QUERY_WG) for f in with_it.flags()), (with_it.flags(), without.flags())
    assert _records(with_it, 0) > 0
    _equal_cells(with_it, without)
    assert with_it.totals() == without.totals() and with_it.results() == without.results()
    # ... and shard_wg alone sets bit 14 without bit 15
    alone = Step(w, qb, 2)
    assert all(f & WALKED and not f & PACKED for f in alone.flags()), alone.flags()
    qb.release()


def test_parity_on_an_unfiltered_world_at_2_ranks(env):
    _parity_unfiltered(env, 2)


# ---- the 4-rank world: rank 1's window [0x40000000, 0x7FFFFFFF] ----------------------------------------------------------------------

M_EDGES = (0, 1, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)


def test_probe_counts_at_every_boundary(env):
    """one batch whose queries hold exactly m distinct hashes of rank 1's window, m at the lane-group (8), wave (64), round (256), pair
    (512) and hq[] (1024) limits and next to them -- real postings' hashes, a doc of the last segment's among them --, padded with
    noise outside the window to n <= 1024 and shuffled; m = 1024 is n = 1024, all in the window"""
    w = _Kept.get(env, 4)
    fpx = w.fpx
    rng = np.random.default_rng(2201)
    lo, hi = w.window(1)
    assert (lo, hi) == (0x40000000, 0x7FFFFFFF)
    pool = Pool(fpx, 4, lo, hi)
    queries, docs, owned = [], [], []
    for k, m in enumerate(M_EDGES):
        doc = LAST + 100 + 37 * k
        inside, n_own = pool.inside(rng, doc, m)
        n = min(PACK_MAX, max(300, m + 100))
        q = np.concatenate([inside, pool.outside(rng, n - m)]).astype(np.uint32)
        rng.shuffle(q)
        assert len(q) == n <= PACK_MAX and pool.count(q) == m, (m, len(q), pool.count(q))       # before any GPU call
        assert n_own >= min(m, 8), (m, n_own)
        queries.append(q); docs.append(doc); owned.append(n_own)
    assert len(queries[-1]) == 1024 and pool.count(queries[-1]) == 1024
    on, _ = _pcompare(w, queries, fpx.SearchOptions(500, 3, 10), 2, rank=1)
    for q, (m, doc, n_own) in enumerate(zip(M_EDGES, docs, owned)):
        if n_own >= 3:                                                # (at or above the floor: the planted doc is a result, by id)
            assert doc in _ids(on.got[q]), (m, doc, on.got[q][:4])
    # rank 1 holds nothing of the query without a hash in its window
    recs, narrow = on.cells()[1][0]
    assert not ((recs & 7 if narrow else recs >> 32) == 0).any()


def _late_queries(fpx, rng, pool, plant=0):
    """six queries whose hashes of the pool's window all sit at raw positions >= 256 (>= 300, 512, 768), every position before them
    outside the window; plant: so many FRESH hashes of the window (no posting of the world's) among each one's late positions, for a
    doc of a memory segment.  -> the queries + 18 ordinary ones, the world's docs aimed at, the fresh hashes per query"""
    queries, docs, fresh = [], [], []
    for k, head in enumerate((256, 256, 256, 300, 512, 768)):
        doc = LAST + 900 + 41 * k
        inside, n_own = pool.inside(rng, doc, 70 + k)
        assert n_own >= 3
        new = (pool.lo + 0x2468 + 15485863 * (np.arange(plant, dtype=np.int64) + plant * k + 1)).astype(np.uint32)
        assert ((new >= pool.lo) & (new <= pool.hi)).all() and not np.isin(new, pool.u).any() and len(np.unique(new)) == plant
        tail = np.concatenate([inside, new, pool.outside(rng, 40)]).astype(np.uint32)
        rng.shuffle(tail)
        q = np.concatenate([pool.outside(rng, head), tail]).astype(np.uint32)
        assert pool.count(q[:head]) == 0 and pool.count(q) == 70 + k + plant and len(q) <= PACK_MAX      # before any GPU call
        queries.append(q); docs.append(doc); fresh.append(new)
    return queries + _queries(fpx)[:18], docs, fresh


def _late_checks(on, docs):
    for q, doc in enumerate(docs):
        assert doc in _ids(on.got[q]), (q, doc, on.got[q][:4])
    recs, narrow = on.cells()[1][0]
    for q in range(len(docs)):                                        # rank 1 has records of every one of them
        assert ((recs & 7 if narrow else recs >> 32) == q).any(), q


def test_positions_change_under_compaction(env):
    """queries whose hashes of rank 1's window all sit at raw positions >= 256 (>= 512, >= 768), the positions before them outside the
    window: after compaction they are the query's FIRST probes -- what reads anything by raw position gets these wrong.  Without
    memory segments (the filtered world); with them: test_positions_change_under_compaction_with_memory_segments below"""
    w = _Kept.get(env, 4)
    fpx = w.fpx
    lo, hi = w.window(1)
    queries, docs, _ = _late_queries(fpx, np.random.default_rng(2202), Pool(fpx, 4, lo, hi))
    on, _ = _pcompare(w, queries, fpx.SearchOptions(500, 3, 10), 2, rank=1)
    _late_checks(on, docs)


def test_duplicates_edges_and_odd_queries(env):
    """one batch: rank 1's win_lo - 1, win_lo, win_hi and win_hi + 1, each the hash of a posting that exists; an empty query; a query
    wholly outside rank 1's window; 0xFFFFFFFF twice; one hash of rank 1's window 40 times; a hash of the window twice, 300 positions
    apart; then ordinary ones -- and the batch's first 1, 7 and 9 queries alone"""
    w = _Kept.get(env, 4)
    fpx = w.fpx
    lo, hi = w.window(1)
    assert (lo - 1, lo, hi, hi + 1) == EDGES
    plain = _queries(fpx)
    outside = plain[20][(plain[20] < lo) | (plain[20] > hi)]
    forty = int(Pool(fpx, 4, lo, hi).own(LAST + 50)[0])                # a hash of rank 1's window with a live posting
    apart = plain[7].copy()
    mine = apart[(apart >= lo) & (apart <= hi)]
    apart = np.concatenate([apart, plain[8][:100]]).astype(np.uint32)  # 400 hashes
    apart[10], apart[310] = mine[0], mine[0]
    assert len(apart) == 400 and lo <= forty <= hi
    queries = [np.array(EDGES + (7, 8), dtype=np.uint32), np.zeros(0, np.uint32), outside, np.array([ONES, ONES], dtype=np.uint32),
               np.full(40, forty, dtype=np.uint32), apart] + plain[:144]
    assert len(outside) > 100 and len(queries) == 150
    opts = fpx.SearchOptions(500, 3, 10)
    for B in (150, 1, 7, 9):
        on, _ = _pcompare(w, queries[:B], opts, 2, rank=1)
        got = on.got
        assert got[0] == [(11, 4), (12, 4), (13, 4)], got[0]           # every edge posting counted once, on the rank that owns its hash
        if B >= 7:
            assert got[1] == [] and got[3] == []                      # (0xFFFFFFFF once after dedup: a score of 1, below the floor)
            cells = on.cells()

            def of_query(r, q):
                recs, narrow = cells[r][0]
                return int(((recs & 7 if narrow else recs >> 32) == q).sum())
            assert of_query(1, 2) == 0                                # rank 1 stored nothing for the query outside its window
            assert of_query(3, 3) == 3                                # the last rank has 0xFFFFFFFF's three docs once each ...
            assert [of_query(r, 3) for r in range(3)] == [0, 0, 0]    # ... and no other rank probed it
            assert [of_query(r, 0) for r in range(4)] == [3, 6, 3, 0]     # the four edge hashes, each on its owner (7 and 8: nobody's postings)
            assert of_query(1, 4) >= 1 and [of_query(r, 4) for r in (0, 2, 3)] == [0, 0, 0]      # forty copies: one probe, on rank 1


@pytest.mark.parametrize("length", [PACK_MAX + 1, DEDUP_MAX])
def test_a_long_query_keeps_the_batch_on_the_window_kernel(env, length):
    """a batch with one query of 1025 (of DEDUP_MAX) hashes runs k_search_window: bit 14 set, bit 15 clear on every rank, bins and
    results equal; the same batch without it packs"""
    w = _Kept.get(env, 4)
    fpx = w.fpx
    rng = np.random.default_rng(length)
    plain = _queries(fpx)[:30]
    long_q = np.concatenate([plain[12][:H], wg.noise(rng, length - H)])
    assert len(long_q) == length
    opts = fpx.SearchOptions(500, 3, 10)
    on, _ = _pcompare(w, plain[:9] + [long_q] + plain[9:], opts, 2, packed=False, rank=1)
    assert all(f & WALKED for f in on.flags())
    _pcompare(w, plain, opts, 2, packed=True, rank=1)


@pytest.mark.parametrize("filtered", [True, False])
def test_positions_change_under_compaction_with_memory_segments(env, filtered):
    """the same late-position queries on a world WITH memory segments -- the filtered world's segments (FILT and MEM, shard_wg 2) and
    the world without re-inserts (MEM alone, shard_wg 1) --: each query also holds ten fresh hashes of rank 1's window among its late
    positions, the ten hashes of a NEW doc in one of two memory segments.  The memory table's filter bit travels with the packed hash
    and the look-up takes the packed hashes: every planted doc is a result with a score of 10, by id"""
    fpx = env[0]
    lo, hi = (1 << 32) // 4, (2 << 32) // 4 - 1
    data = _world_data(fpx, np.random.default_rng(4), edges=True, again=filtered)
    pool = Pool(fpx, 4, lo, hi, data)
    queries, docs, fresh = _late_queries(fpx, np.random.default_rng(2203), pool, plant=10)
    planted = [S * PER + 900 + k for k in range(len(docs))]
    changes = [[("insert", planted[k], [int(h) for h in fresh[k]]) for k in range(len(docs)) if k % 2 == m] for m in range(2)]
    assert all(changes)
    with _made(env, 4, data, changes) as w:
        assert w.window(1) == (lo, hi)
        on, _ = _pcompare(w, queries, fpx.SearchOptions(500, 3, 10), 2 if filtered else 1, rank=1)
        _late_checks(on, docs)
        for q, doc in enumerate(planted):
            assert (doc, 10) in on.got[q], (q, doc, on.got[q][:4])


# ---- 8 ranks: m (about 37) far below a round, waves 1 - 3 skip ------------------------------------------------------------------------

def test_parity_on_a_filtered_world_at_8_ranks(env):
    _parity(env, 8)


def test_parity_on_an_unfiltered_world_at_8_ranks(env):
    _parity_unfiltered(env, 8)


# ---- memory segments --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 8])
def test_memory_segments_behind_their_table(env, world):
    """test_gpu_shard_wg.py's shape -- two memory segments that write 50 docs again, with hashes of the batch's queries, and delete 10
    (FILT and MEM) -- plus eight NEW docs in the memory segments whose ten hashes each lie in rank 1's window and stand in their query at
    raw positions 260 .. 269 only: the memory table's filter bit and its look-up must follow the hash to its packed place.  Their docs
    are results, by id and score"""
    fpx = env[0]
    queries = [q.copy() for q in _queries(fpx)]
    rng = np.random.default_rng(50 + world)
    lo, hi = (1 << 32) // world, (2 << 32) // world - 1               # rank 1's window
    planted = {}
    for k in range(8):
        qi, doc = 9 + 13 * k, S * PER + 500 + k
        hs = (lo + 0x1234 + 7919 * (np.arange(10, dtype=np.int64) + 10 * k) * 257).astype(np.uint32)
        assert ((hs >= lo) & (hs <= hi)).all() and not np.isin(hs, queries[qi]).any() and len(np.unique(hs)) == 10
        assert len(queries[qi]) >= 270
        queries[qi][260:270] = hs
        assert not np.isin(hs, queries[qi][:256]).any()
        planted[qi] = (doc, hs)
    docs = rng.choice(np.arange(1, S * PER, dtype=np.int64), 60, replace=False)
    changes = []
    for m in range(2):
        again, gone = docs[m * 25:(m + 1) * 25], docs[50 + m * 5:55 + m * 5]
        changes.append([("insert", int(d), [int(h) for h in queries[(7 * i + m) % 150][:40 + i]]) for i, d in enumerate(again)] +
                       [("delete", int(d)) for d in gone] +
                       [("insert", doc, [int(h) for h in hs]) for qi, (doc, hs) in planted.items() if qi % 2 == m])
    with _made(env, world, _world_data(fpx, np.random.default_rng(world), again=False), changes) as w:
        assert w.window(1) == (lo, hi)
        for opts in (fpx.SearchOptions(500, 3, 10), fpx.http_options()):
            on, _ = _pcompare(w, queries, opts, 2, rank=1)
            if opts.max_results == 500:                               # (room for every doc at or above the floor)
                for qi, (doc, hs) in planted.items():
                    assert (doc, 10) in on.got[qi], (qi, doc, on.got[qi][:4])


def test_memory_segments_of_new_docs_on_an_unfiltered_group(env):
    """memory segments that only ADD docs leave the group unfiltered: shard_wg 1 packs it with the table (MEM without FILT).  The new docs'
    hashes stand at raw positions >= 256 of their queries, in rank 1 of 2's window"""
    fpx = env[0]
    queries = [q.copy() for q in _queries(fpx)]
    lo, hi = 1 << 31, (1 << 32) - 1
    planted = {}
    for k in range(6):
        qi, doc = 4 + 11 * k, S * PER + 700 + k
        hs = (lo + 0x4321 + 104729 * (np.arange(12, dtype=np.int64) + 12 * k) * 131).astype(np.uint32)
        assert ((hs >= lo) & (hs <= hi)).all() and not np.isin(hs, queries[qi]).any() and len(np.unique(hs)) == 12
        assert len(queries[qi]) >= 292
        queries[qi][280:292] = hs
        planted[qi] = (doc, hs)
    changes = [[("insert", doc, [int(h) for h in hs]) for qi, (doc, hs) in planted.items() if qi % 2 == m] for m in range(2)]
    assert all(changes)
    with _made(env, 2, _world_data(fpx, np.random.default_rng(2), again=False), changes) as w:
        on, _ = _pcompare(w, queries, fpx.SearchOptions(500, 3, 10), 1, rank=1)
        for qi, (doc, hs) in planted.items():
            assert (doc, 12) in on.got[qi], (qi, doc, on.got[qi][:4])


# ---- a query whose records outgrow the workgroup's array: the same call is answered by the pipeline, and the next 32 -------------------

def test_hand_back_and_back_off(env):
    """test_gpu_shard_wg.py's shape under shard_pack 1: a query of exactly 8192 records in rank 0's window is packed and walked; one of
    8193 hands rank 0's step to the pipeline inside the call -- today's flags, neither bit 14 nor 15 -- and rank 0's snapshot stays
    there for its next 32 calls; the 33rd packs again.  Rank 1 packs throughout"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(1540)
    single0 = 0x70000000
    singles = np.array([single0 + 7919 * k for k in range(3500)], dtype=np.uint32)
    data = []
    for s in range(8):
        ids = np.arange(1 + s * 1200, 1 + (s + 1) * 1200, dtype=np.int64)
        extra = [(HOT8, ids[:1000])]
        if s == 0:
            extra.append((HOT1, ids[200:1200]))
        if s == 1:
            extra += [(int(h), ids[i % len(ids): i % len(ids) + 1]) for i, h in enumerate(singles)]
        data.append((wg.rand_items(rng, ids, 24, extra), int(ids.min()), int(ids.max()), ids.astype(np.uint32), None))
    with _made(env, 2, data) as w:
        assert max(HOT8, HOT1, int(singles.max())) <= w.window(0)[1]

        def records(p, q):                                            # the records rank 0's window gives the query
            return p.osnap.search(q[q <= w.window(0)[1]], 40, 1, 0, with_stats=True)[1].scanned_docs
        exact = functools.partial(wg.exact, records)
        items = [d[0] for d in data]
        plain = [wg.aimed(rng, items[i % 8], 300) for i in range(30)]
        plain = [q[(q != HOT8) & (q != HOT1)] for q in plain]
        fits, over = exact(w.full, rng, [HOT8], singles, 8192), exact(w.full, rng, [HOT8], singles, 8193)
        assert (records(w.full, fits), records(w.full, over)) == (8192, 8193) and max(len(fits), len(over)) <= PACK_MAX
        opts = fpx.SearchOptions(500, 3, 10)
        light = plain[:11] + [fits] + plain[11:]
        heavy = light[:20] + [over] + light[20:]
        on, _ = _pcompare(w, light, opts, 1, cell_cap=8192)           # 8192 records: packed on both ranks
        assert on.attempts == 1
        # call 1: 8193 records -- the call succeeds, the pipeline answered on rank 0; calls 2 .. 33 on rank 0's snapshot stay there
        on, _ = _pcompare(w, heavy, opts, 1, packed=[False, True], walked=[False, True], cell_cap=8192)
        assert on.attempts == 1 and not on.flags()[0] & (PACKED | WALKED | QUERY_WG) and on.flags()[0] & 16
        import torch
        qb = fpx.QueryBatch(ctx, light, opts)
        bpr = fpx.shard_bins_per_rank(qb.B, 2)
        send = torch.zeros((2, bpr, 8192), dtype=torch.int64, device="cuda")
        counts = torch.zeros((2, bpr), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.set_option("shard_wg", 1)
        ctx.set_option("shard_pack", 1)
        seen = []
        for call in range(2, 35):
            st, need = fpx.shard_probe(w.readers[0], qb, 2, send.data_ptr(), 8192, counts.data_ptr())
            assert st is not None, need
            assert bool(st.path_flags & PACKED) == bool(st.path_flags & WALKED)
            seen.append(bool(st.path_flags & PACKED))
        assert seen == [False] * 32 + [True], seen                    # calls 2 .. 33 clear, call 34 packs again
        st, _ = fpx.shard_probe(w.readers[1], qb, 2, send.data_ptr(), 8192, counts.data_ptr())
        assert st.path_flags & ALL_FOUR == ALL_FOUR
        qb.release()


# ---- the one call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 4])
def test_one_call_over_window_sharded_contexts(env, world):
    """fpx_sharded_search_batch over `world` window-sharded contexts with shard_wg 2 and shard_pack 1 on every context: results == the
    unsharded reader's == the oracle's, the unsharded statistics, bit 15 in the returned flags; with shard_pack 1 on all contexts but
    one the results are the same and bit 15 is clear (bit 14 stays: every rank walked)"""
    fpx, oracle, Pair, ctx0 = env
    import torch
    _Kept.drop()
    ndev = torch.cuda.device_count()
    ctxs = [fpx.Context(k % ndev) for k in range(world)]
    for c in ctxs:
        c.set_option("direct", 1); c.set_option("direct_min_items", 0); c.set_option("fuse_min", 1); c.set_option("group_packed", 1)
    full = Pair(ctxs[0])
    slices = [[] for _ in range(world)]
    for s, (items, lo, hi, ids, alive) in enumerate(_world_data(fpx, np.random.default_rng(world))):
        blocks, index = full.add_file(items, lo, hi, s + 1, ids, alive)
        for k, sl in enumerate(fpx.file_segment_windows(ctxs, blocks, 512, index, lo, hi, s + 1, ids, alive)):
            slices[k].append(sl)
    full.finish()
    sh = fpx.ShardedIndexReader(fpx.WindowShardedSegments(ctxs, slices))
    try:
        assert sh.snapshot.num_devices == world
        queries = _queries(fpx)
        for opts in _three(fpx)[:2]:
            want, wst = full.check(queries, opts, with_stats=False)
            assert any(want)
            # (shard_wg, shard_pack on every context but the last, on the last) -> bits 14 and 15
            for wgv, pack, pack_last, walked, packed in ((2, 1, 1, True, True), (2, 1, 0, True, False), (0, 1, 1, False, False), (2, 1, 1, True, True)):
                for k, c in enumerate(ctxs):
                    c.set_option("shard_wg", wgv)
                    c.set_option("shard_pack", pack_last if k == world - 1 else pack)
                got, st = sh.search_batch(queries, opts)
                print(f"shard_wg {wgv}, shard_pack {pack} / {pack_last}: path_flags {st.path_flags}")
                assert got == want
                assert bool(st.path_flags & WALKED) == walked and bool(st.path_flags & PACKED) == packed and st.path_flags & 16
                assert (st.scanned_blocks, st.scanned_docs, st.probes, st.hits) == (wst.scanned_blocks, wst.scanned_docs, wst.probes, wst.hits)
    finally:
        sh.snapshot.release()
        full.reader.snapshot.release()
        for g in [g for row in slices for g in row] + full.gpu_segs:
            g.release()
        for c in ctxs:
            c.trim()
