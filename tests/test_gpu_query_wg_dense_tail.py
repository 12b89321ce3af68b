"""The exact count of k_search_query's tail (csrc/fpx_qsearch.hpp), DENSE: a sweep over the records leaves a bit per record whose filter
cell reaches the floor in the lane's mask -- bit 4 turn + u for record turn * 1024 + 4 lane + u --, a drain then takes a lane's bits one
by one into the exact table, once per pass.  What can go wrong there: a bit not cleared or not re-armed for a second pass, a record read
back from the wrong place, the last turn's bound, bits 28 .. 31.

Every case is a batch on a tiny packed group (wg_harness.py's World) through both(): Pair.check against the oracle under the option, then
the batch under the option and under 0, results, statistics, per-query blocks / docs and histograms compared.  (The redone query compares
results and statistics by hand: under hot_wg = 0 its batch is handed back, and the back-off that follows is drained.)

The worlds keep their random hashes in [WORDS_LO, WORDS_HI) and the made hashes below: a query's record count is what it is made for
(asserted against the oracle's count).  Column 0 holds the docs that are looked for, the other columns the fill: PAIR hashes of two docs
each and SINGLE hashes of one.

WHERE a record lands in the workgroup's array is decided by LDS atomics between the waves; it is fixed only for a query of at most 64
hashes without lists or words in `ext`: one wave's round, its records placed lane by lane by the reservation's scan -- lane 8 g + sub has
words 4 sub .. 4 sub + 3 of the lines of its group's eight hashes, line by line.  Two cases are made for that:

* one_lane: four hashes at positions 0 .. 3 of the query, each the first hash value of a line of its own, each T3's alone: records 0 .. 3
  are lane 0's words of lines 0 .. 3, every survivor of the array in lane 0's bits 0 .. 3.
* test_one_lane_owns_the_survivors_of_two_turns (sixteen-column lines): T's eight hashes at positions 0 .. 3 and 48 .. 51 of a query of 64,
  between them hashes of 28 words (fourteen doubles) and one of 12 that make the records before group 6 exactly 1024: records 0 .. 3 and
  1024 .. 1027 are T's, bits 0 .. 7 of lane 0 of the tail -- the first four records of BOTH turns of a query of 1028 records -- and nobody
  else has a survivor (unless a fill doc shares T's filter cell).  The places follow from the kernel's layout as described; no test can read them.

Every turn of one lane cannot be pinned that way (64 hashes of at most 28 inline words are 1792 records).  What `crowded` fixes instead: 36
hashes of the same 200 docs, 7200 records that ALL reach the floor -- every lane's mask is full, 28 bits and 32 for the lanes of the eighth
turn's 32 records, the drain makes the maximum number of trips per pass, and the table doubles its passes over full masks.  `long` has its
600 survivors in the last records (lists join the array last): about four bits per lane in turns 6 and 7, bits 28 .. 31 for eight lanes.
For the record counts 1023 .. 4097 "first" and "last" say where the target's hashes stand in the query, which decides the place of its
records only loosely."""
import numpy as np
import pytest

import wg_harness as wg
from wg_harness import FILTERED, GROUP, LOW, QUERY_WG, REDONE, WORDS_LO, WORDS_HI, noise as _noise, rand_items as _rand_items

pytestmark = pytest.mark.gpu

OPTIONS = ("query_wg", "hot_wg", "low_wg", "direct_min_items")
TGT, LANE, CROWD, SINGLE, PAIR, HOT, MEMT = 0x01000000, 0x02000000, 0x03000000, 0x04000000, 0x05000000, 0x06000000, 0x07000000
NSINGLE = 40
COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 4097)
QS_WG = 256


def _h(base, i):
    """made hash number i of a kind: a line of its own (64 hash values apart), the line's first hash value"""
    return base + 64 * i


class Made:
    """the docs and hashes of a world: T1, T2 (three hashes each), T3 (four), a crowd of 200 docs under 36 hashes (crowd_h: the first three), in column 0;
    in every other column `npair` PAIR hashes of two docs each, NSINGLE SINGLE hashes of one, three HOT hashes of all its docs"""

    def __init__(self, cols, per, first=1):
        self.cols, self.per, self.first = cols, per, first
        self.npair = (per - NSINGLE) // 2
        self.t1, self.t2, self.t3 = first, first + 1, first + 2
        self.h1 = np.array([_h(TGT, j) for j in range(3)], dtype=np.uint32)
        self.h2 = np.array([_h(TGT, 8 + j) for j in range(3)], dtype=np.uint32)
        self.h3 = np.array([_h(LANE, j) for j in range(4)], dtype=np.uint32)
        self.crowd_all = np.array([_h(CROWD, j) for j in range(36)], dtype=np.uint32)
        self.crowd_h = self.crowd_all[:3]
        self.crowd = list(range(first + 100, first + 300))
        self.hot = np.array([_h(HOT, j) for j in range(3)], dtype=np.uint32)
        self.pairs = np.array([_h(PAIR, (s - 1) * self.npair + i) for s in range(1, cols) for i in range(self.npair)], dtype=np.uint32)
        self.singles = np.array([_h(SINGLE, (s - 1) * NSINGLE + i) for s in range(1, cols) for i in range(NSINGLE)], dtype=np.uint32)

    def extra(self, s, ids):
        if s == 0:
            return ([(int(h), ids[0:1]) for h in self.h1] + [(int(h), ids[1:2]) for h in self.h2] + [(int(h), ids[2:3]) for h in self.h3]
                    + [(int(h), ids[100:300]) for h in self.crowd_all])
        out = [(_h(PAIR, (s - 1) * self.npair + i), ids[2 * i: 2 * i + 2]) for i in range(self.npair)]
        out += [(_h(SINGLE, (s - 1) * NSINGLE + i), ids[2 * self.npair + i: 2 * self.npair + i + 1]) for i in range(NSINGLE)]
        return out + [(int(h), ids) for h in self.hot]

    def fill(self, n, skip=0):
        """hashes that give exactly n records, every doc once: pairs from number `skip` on, then a single"""
        assert n // 2 + skip <= len(self.pairs)
        return np.concatenate([self.pairs[skip: skip + n // 2], self.singles[: n % 2]])


def _world(Pair, ctx, rng, cols, per, **kw):
    m = Made(cols, per)
    w = wg.World(Pair, ctx, packed=1, lo=WORDS_LO, hi=WORDS_HI, **kw)
    return m, w


def _records(p, q):
    return p.osnap.search(q, 40, None, 10, with_stats=True)[1].scanned_docs


def _opts(fpx, floor, k=500):
    return fpx.SearchOptions(max_results=k, min_score=floor, min_score_pct=0)


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.fixture
def tiny(env, monkeypatch):
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1) as e:
        yield e


def _cases(fpx, m, rng, p, counted=True):
    """-> [(name, query, options, expected results or None, records or None)]; counted: the record counts are asserted (a doc written
    again is two records until the newer column supersedes the older)"""
    cases = []
    # one lane owns all survivors: records 0 .. 3 are T3's, nothing else reaches 4
    cases.append(("one_lane", np.concatenate([m.h3, _noise(rng, 60)]), _opts(fpx, 4), [(m.t3, 4)], None))
    cases.append(("one_lane_among_fill", np.concatenate([m.h3, m.fill(40, skip=7)[:20], _noise(rng, 40)]), _opts(fpx, 4), [(m.t3, 4)], None))
    # no survivors: 300 records of 300 docs, a floor of 50
    cases.append(("no_survivors", m.fill(300), _opts(fpx, 50), [], 300))
    # odd record counts
    for n in COUNTS:
        for mode in ("none", "first", "last", "both"):
            tgt = {"none": 0, "first": 3, "last": 3, "both": 6}[mode]
            if (mode == "none") != (n < 3) or n < tgt or (mode == "last" and n == 3):
                continue
            q = np.concatenate([m.h1 if mode in ("first", "both") else m.h1[:0], m.fill(n - tgt, skip=n % 11), m.h2 if mode in ("last", "both") else m.h2[:0]])
            want = [(m.t1, 3)] * (mode in ("first", "both")) + [(m.t2, 3)] * (mode in ("last", "both"))
            cases.append((f"count_{n}_{mode}", q, _opts(fpx, 3), want, n))
    # the table doubles its passes: 200 docs at the floor of 3
    crowd = [(d, 3) for d in m.crowd]
    cases.append(("doubling", np.concatenate([m.crowd_h, m.fill(200)]), _opts(fpx, 3), crowd, 800))
    # more than seven turns of records, the survivors -- lists: they join the array last -- in the eighth
    nlong = 7 * 4 * QS_WG + 270
    cases.append(("long", np.concatenate([m.fill(nlong - 600), m.crowd_h]), _opts(fpx, 3), crowd, nlong))
    # every record a survivor: full masks in every lane, eight turns, the passes doubled
    cases.append(("crowded", m.crowd_all, _opts(fpx, 3), [(d, 36) for d in m.crowd], 7200))
    for name, q, o, want, n in cases:
        assert n is None or not counted or _records(p, q) == n, (name, n, _records(p, q))
    return cases


def _expect(cases, got):
    for (name, q, o, want, n), g in zip(cases, got):
        if want is not None:
            assert sorted(g) == sorted(want), (name, g[:5], want[:5])


@pytest.mark.parametrize("cols", [9, 5])
def test_the_dense_tail(tiny, cols):
    """lines of 4 hash values (9 columns: the sixteen-column instantiation, the headline's) and of 8 (5 columns)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1900 + cols)
    m, w = _world(Pair, ctx, rng, cols, 900 if cols == 9 else 1800)
    p, _ = w.columns(rng, cols, m.per, 40, m.extra)
    cases = _cases(fpx, m, rng, p)
    assert len(cases) <= 64 and {c[0] for c in cases} >= {"count_1_none", "count_3_first", "count_5_last", "count_4097_both", "long", "crowded"}
    got, st = wg.both(ctx, p, [c[1] for c in cases], [c[2] for c in cases], "query_wg", 1, clear=QUERY_WG, want=QUERY_WG | GROUP, want_not=FILTERED)
    _expect(cases, got)


def test_next_to_a_memory_segment(tiny):
    """MEM: a doc of a memory segment under T1's hashes and three of its own; the group's cases beside it"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1910)
    m, w = _world(Pair, ctx, rng, 5, 1800)
    w.columns(rng, 5, m.per, 40, m.extra)
    ids = np.arange(5 * m.per + 1, 5 * m.per + 41)
    hm = np.array([_h(MEMT, j) for j in range(3)], dtype=np.uint32)
    w.memory(_rand_items(rng, ids, 40, [(int(h), ids[:1]) for h in hm] + [(int(h), ids[1:2]) for h in m.h1], WORDS_LO, WORDS_HI), ids)
    p = w.finish()
    assert p.reader.snapshot.info()["memory"] == 1
    mem, both_ = [(int(ids[0]), 3)], [(m.t1, 3), (int(ids[1]), 3)]
    cases = [("mem_alone", np.concatenate([hm, m.fill(1021)]), _opts(fpx, 3), mem, None),
             ("mem_and_group", np.concatenate([m.fill(1019), m.h1, hm]), _opts(fpx, 3), mem + both_, None),
             ("mem_crowd", np.concatenate([m.crowd_h, m.fill(200), m.h1]), _opts(fpx, 3), [(d, 3) for d in m.crowd] + both_, None),
             ("mem_none", m.fill(300), _opts(fpx, 50), [], None)]
    got, st = wg.both(ctx, p, [c[1] for c in cases], [c[2] for c in cases], "query_wg", 1, clear=QUERY_WG, want=QUERY_WG | GROUP, want_not=FILTERED)
    _expect(cases, got)


def test_on_a_filtered_group(env, monkeypatch):
    """query_wg = 2: T1 written again by the newest column with its own hashes -- found once, there"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1):
        fpx, oracle, Pair, ctx = env
        rng = np.random.default_rng(1920)
        m, w = _world(Pair, ctx, rng, 5, 1800, snapshot_query_wg=2)
        p, _ = w.columns(rng, 5, m.per, 40, m.extra, again={m.t1: None})
        cases = _cases(fpx, m, rng, p, counted=False)
        got, st = wg.both(ctx, p, [c[1] for c in cases], [c[2] for c in cases], "query_wg", 2, clear=QUERY_WG, want=QUERY_WG | GROUP | FILTERED)
        _expect(cases, got)


def test_a_low_floor_among_default_ones(tiny):
    """low_wg = 1: the query with a floor of 1 takes the sorted tail, its neighbours the dense one"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1930)
    m, w = _world(Pair, ctx, rng, 5, 1800)
    p, _ = w.columns(rng, 5, m.per, 40, m.extra)
    cases = [c for c in _cases(fpx, m, rng, p) if c[0] in ("one_lane", "no_survivors", "count_1025_both", "count_5_last", "doubling", "long", "crowded")]
    low = np.concatenate([m.h1, m.fill(200, skip=3), m.h2])
    cases.insert(2, ("low", low, _opts(fpx, 1, k=2), [(m.t1, 3), (m.t2, 3)], 206))
    cases.append(("low_again", low[::-1].copy(), _opts(fpx, 2, k=500), [(m.t1, 3), (m.t2, 3)], None))
    got, st = wg.both(ctx, p, [c[1] for c in cases], [c[2] for c in cases], "low_wg", 1, clear=LOW | QUERY_WG, want=LOW | QUERY_WG | GROUP)
    _expect(cases, got)


def test_a_redone_query(tiny):
    """hot_wg = 1: three hashes of every doc of four columns -- 21600 records -- beside the crowd; the query is redone in doc classes, each
    class through the dense tail with its passes doubled.  Under hot_wg = 0 the batch is handed back, as before: the same results"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1940)
    m, w = _world(Pair, ctx, rng, 5, 1800)
    p, _ = w.columns(rng, 5, m.per, 40, m.extra)
    plain = [np.concatenate([m.h1, m.fill(500, skip=i), _noise(rng, 100)]) for i in range(8)]
    heavy = list(plain)
    heavy[3] = np.concatenate([m.hot, m.crowd_h, m.h2, m.fill(100)])
    assert _records(p, heavy[3]) > wg.QS_REC_CAP
    opts = _opts(fpx, 3, k=100)
    try:
        ctx.set_option("hot_wg", 1)
        got, st = p.check(heavy, opts)
        assert st.path_flags & (QUERY_WG | REDONE) == QUERY_WG | REDONE, st.path_flags
        g1, s1 = p.reader.search_batch(heavy, opts)
        ctx.set_option("hot_wg", 0)
        g0, s0 = p.reader.search_batch(heavy, opts)
        assert not s0.path_flags & REDONE, s0.path_flags
        for _ in range(40):                                   # (the snapshot's back-off after the hand-back)
            if p.reader.search_batch(plain, opts)[1].path_flags & QUERY_WG:
                break
        else:
            raise AssertionError("the query-per-workgroup path did not come back")
    finally:
        ctx.set_option("hot_wg", -1)
    assert g1 == got and g0 == got
    assert wg.figures(s1)[:wg.FOUR] == wg.figures(s0)[:wg.FOUR] == wg.figures(st)[:wg.FOUR]
    assert len(got[3]) == 100 and all(s >= 3 for _, s in got[3])      # (the hot docs, the fill's among them at 4)
    assert all(g == [(m.t1, 3)] for i, g in enumerate(got) if i != 3)


def test_one_lane_owns_the_survivors_of_two_turns(tiny):
    """records 0 .. 3 and 1024 .. 1027 of a query of 1028 records are T's (the module's docstring says how they are pinned): the drain
    takes eight bits of one lane's mask, four of each turn, while the other lanes idle.  Fifteen columns: the sixteen-column instantiation"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1950)
    ta = np.array([_h(TGT, j) for j in range(4)], dtype=np.uint32)
    tb = np.array([_h(TGT, 8 + j) for j in range(4)], dtype=np.uint32)
    fills = np.array([_h(PAIR, i) for i in range(36)], dtype=np.uint32)       # 28 words each: a double in each of columns 1 .. 14
    twelve = _h(SINGLE, 0)                                                      # 12 words: a doc in each of columns 1 .. 12

    def extra(s, ids):
        if s == 0:
            return [(int(h), ids[0:1]) for h in np.concatenate([ta, tb])]
        return [(int(h), ids[2 * i: 2 * i + 2]) for i, h in enumerate(fills)] + ([(twelve, ids[150:151])] if s <= 12 else [])

    w = wg.World(Pair, ctx, packed=1, lo=WORDS_LO, hi=WORDS_HI)
    p, _ = w.columns(rng, 15, 200, 40, extra)
    q = np.concatenate([ta, fills[:4], fills[4:36], np.array([twelve], dtype=np.uint32), _noise(rng, 7), tb, _noise(rng, 12)])
    assert len(q) == 64 and list(q[48:52]) == list(tb)
    assert 4 + 4 * 28 + 32 * 28 + 12 == 4 * QS_WG                              # the records before group 6: one turn, exactly
    other = np.concatenate([tb, fills[::-1], ta])                               # (the same records, their places not pinned)
    assert _records(p, q) == 4 * QS_WG + 4 and _records(p, other) == 8 + 36 * 28
    got, st = wg.both(ctx, p, [q, other, q], _opts(fpx, 8), "query_wg", 1, clear=QUERY_WG, want=QUERY_WG | GROUP, want_not=FILTERED)
    assert got == [[(1, 8)]] * 3, got
