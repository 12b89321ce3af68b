"""Option groups_wg = 2 with low_wg (csrc/fpx_qsearch.hpp: k_search_low_next): a batch with queries whose score floor is 1 or 2 -- the
legacy protocol's min_score 1, the default floor of a query of 40 hashes or fewer -- on a snapshot of SEVERAL packed groups stays on the
query-per-workgroup path: k_search_low (k_search_low_filt on a filtered group) over the first group, k_search_low_next over the others --
the sorted tail for the low-floor queries, the usual one for the batch's others, the chained hand-over behind either --, one k_finish.
fpx_stats.path_flags: bits 13 (8192) and 12 (4096) together, with bit 6 (64) a query per workgroup and bit 2 (4) a group; bit 8 (256)
when any group is filtered, bit 7 (128) two parts, bit 1 (2) the shared candidate list.

Every case goes through wg_harness.both(): Pair.check under groups_wg = 2 and low_wg = 1 (2 for filtered groups) -- results and every
query's scanned blocks / docs == the oracle's -- with the path bits asserted, then the batch under groups_wg 2 and under 0 compared:
results, scanned_blocks, scanned_docs, probes, hits, algorithmic_bytes, per-query blocks / docs and the growth of the scan histograms.
Under 0 such a batch is the pipeline's: bits 13 and 12 clear.  Snapshots are made under groups_wg = 2 (the option also decides, when a
snapshot is made, which groups are its part 0).  A second group is made the way tests/test_gpu_groups_wg.py makes one, whose helpers
_more, _finish and _layout are imported.  The worlds are a few thousand docs x 40 hashes, each case the smallest shape that reaches its
branch.  On a library without the feature groups_wg = 2 means 0: every case fails at the path bits."""
import functools

import numpy as np
import pytest

import wg_harness as wg
from test_gpu_groups_wg import _finish, _layout, _more
from wg_harness import (FILTERED, GROUP, LOW, QS_MAX_HASHES, QS_REC_CAP, QUERY_WG, SECOND_TRIP, TWO_PARTS, HOT8, HOT1,
                        aimed as _aimed, legacy as _legacy, noise as _noise, rand_items as _rand_items, rows as _rows, sampled as _sampled)

pytestmark = pytest.mark.gpu

GROUPS = 8192                       # fpx_stats.path_flags bit 13
TAKEN = GROUPS | LOW | QUERY_WG | GROUP
OPTIONS = ("groups_wg", "query_wg", "low_wg", "hot_wg", "direct_min_items")
SHARED, DOUBLE, CROWD, SINGLE, HAND, HOTB, BIG = 0x2BADF00D, 0x37770000, 0x51515151, 0x70000000, 0x61000000, 0x4BCDEF01, 0x63000000
OTHER = (0x2C0FFEE1, 0x2D0FFEE3)    # a hash that lists 11 docs of group 0 / of group 1
_usual = wg.usual(SHARED, DOUBLE)


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.fixture
def tiny(env, monkeypatch):
    """every file segment a direct-addressed candidate unless a test says otherwise, groups packed"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1) as e:
        yield e


def _both(ctx, p, queries, opts, want=TAKEN, want_not=0, low_wg=1, also=()):
    """Pair.check under groups_wg = 2 and low_wg with the path bits asserted, then the batch under groups_wg 2 and under 0, everything equal"""
    return wg.both(ctx, p, queries, opts, "groups_wg", 2, clear=GROUPS | LOW, want=want, want_not=want_not,
                   also=(("low_wg", low_wg),) + tuple(also), compare=wg.WITH_BYTES)


def _two_groups(Pair, ctx, rng, cols0=4, cols1=2, per0=800, per1=600, extra0=_usual, extra1=lambda s, ids: [], first=1, **kw):
    """-> the world, the second group's first doc, the first free doc"""
    w = wg.World(Pair, ctx, **kw)
    _, nxt = w.columns(rng, cols0, per0, 40, extra0, first=first)
    return w, nxt, _more(w, rng, cols1, per1, 40, nxt, extra1)


def _queries(rng, w, n, qlen=400):
    """queries aimed at docs of the world's segments in turn"""
    return [_aimed(rng, w.items[i % len(w.items)], qlen, [SHARED, DOUBLE][: i % 3]) for i in range(n)]


# ---- 1. the legacy options on two clean groups ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [(5, 2), (9, 3), (3, 9)])
def test_legacy_options_on_two_clean_groups(tiny, cols):
    """5 + 2 columns (both of 8-column lines), 9 + 3 and 3 + 9 (the launches' NS differ); 24 queries of 1000 hashes aimed at docs of both
    groups.  Every third one also holds a hash that lists 11 docs of the OTHER group: there the query's best score is 1, that launch's
    raised floor stays 1 and it hands the eleven over -- k_finish's cut, from the target's 40 in the other group, drops them.  The first
    test of the file: on the parent the path bits are the pipeline's"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2000 + 16 * cols[0] + cols[1])
    per = 1200 if cols == (5, 2) else 500
    w, end0, _ = _two_groups(Pair, ctx, rng, cols[0], cols[1], per, per,
                             lambda s, ids: _usual(s, ids) + ([(OTHER[0], ids[:11])] if s == 0 else []),
                             lambda s, ids: _usual(s, ids) + ([(OTHER[1], ids[:11])] if s == 0 else []))
    p = _finish(w, 2)
    assert _layout(p) == [(c, 8 if c <= 8 else 16, 1) for c in cols], _layout(p)
    info = p.reader.snapshot.info()
    assert info["groups"] == 2 and info["packed_groups"] == 2, info
    ncols, queries, crossed = cols[0] + cols[1], [], []
    for i in range(24):
        s = (i * 5) % ncols                                  # (the target's column)
        cross = i % 3 == 0
        queries.append(_aimed(rng, w.items[s], 1000, [OTHER[1 if s < cols[0] else 0]] if cross else [SHARED, DOUBLE][: i % 2]))
        if cross:
            crossed.append(i)
    got, st = _both(ctx, p, queries, _legacy(fpx), want_not=TWO_PARTS | FILTERED)
    best = [g[0][0] for g in got]
    assert all(g and g[0][1] >= 20 for g in got), [g[:1] for g in got]
    assert sum(1 for d in best if d < end0) >= 3 and sum(1 for d in best if d >= end0) >= 3, best
    for i in crossed:                                          # (the other group's eleven, at a score of 1 -- 2 or 3 where a doc is on one of the target's shared lists too: handed over, cut)
        full = dict(p.osnap.search(queries[i], 500, 1, 0))
        other = [d for d in full if (d >= end0) != (best[i] >= end0)]
        assert len(other) >= 11 and max(full[d] for d in other) <= 3, (i, [(d, full[d]) for d in other[:12]])
        assert all(s >= 4 for _, s in got[i]) and not set(other) & {d for d, _ in got[i]}, got[i][:3]
    # off by default: the pipeline
    _, st_d = p.reader.search_batch(queries, _legacy(fpx))
    assert not st_d.path_flags & (GROUPS | LOW | QUERY_WG) and st_d.path_flags & GROUP, st_d.path_flags


# ---- 2. nothing raises the floor --------------------------------------------------------------------------------------------------------

def _crowd(Pair, ctx, rng, ngroups, n):
    """`ngroups` groups of 3 / 2 / 2 columns of 600 docs; `n` docs of each group's first column (ids[100 : 100 + n]) share thirty hashes"""
    hashes = np.array([CROWD + k * 7919 for k in range(30)], dtype=np.uint32)
    extra = lambda s, ids: [(int(c), ids[100:100 + n]) for c in hashes] if s == 0 else []
    w = wg.World(Pair, ctx)
    firsts = [1]
    _, nxt = w.columns(rng, 3, 600, 40, extra)
    for gi in range(1, ngroups):
        if gi == 2:
            w.finish()                                         # (a third group: by a third snapshot)
        firsts.append(nxt)
        nxt = _more(w, rng, 2, 600, 40, nxt, extra)
    p = _finish(w, 2)
    assert _layout(p) == [(3, 8, 1)] + [(2, 8, 1)] * (ngroups - 1), _layout(p)
    return w, p, hashes, firsts


def test_nothing_raises_the_floor(tiny):
    """60 docs of each group's first column share thirty hashes: a tie at 30 ACROSS the groups.  min_score_pct 0, min_score 1 and 2,
    limits 1, 7, 100 and 500: every launch hands over its own group's top `limit`, k_finish takes the lowest ids of the tie -- limit 100:
    the 60 of the lower-id group and the 40 lowest of the other; the hundreds of docs at a score of 1 that the sampled hashes give are the
    tie at the cut for limit 500"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2010)
    w, p, hashes, firsts = _crowd(Pair, ctx, rng, 2, 60)
    rest = np.concatenate(w.items[1:3] + w.items[4:])          # (the sampled hashes stay off the crowds' columns: the tie stays a tie)
    sets = [fpx.SearchOptions(max_results=k, min_score=m, min_score_pct=0) for m in (1, 2) for k in (1, 7, 100, 500)]
    queries, opts = [], []
    for i in range(16):
        q = np.concatenate([hashes, _sampled(rng, rest, 900), _noise(rng, 100)])
        rng.shuffle(q)
        queries.append(q)
        opts.append(sets[i % 8])
    got, st = _both(ctx, p, queries, opts, want=TAKEN | SECOND_TRIP)
    tie = [firsts[0] + 100 + i for i in range(60)] + [firsts[1] + 100 + i for i in range(60)]
    assert got[0] == [(tie[0], 30)] and got[1] == [(d, 30) for d in tie[:7]], (got[0], got[1])
    assert got[2] == [(d, 30) for d in tie[:100]] and got[6] == got[2], got[2][58:62]
    assert len(got[3]) == 500 and got[3][:120] == [(d, 30) for d in tie] and got[3][-1][1] == 1, got[3][118:122]


def test_three_groups_and_three_hundred_candidates(tiny):
    """three groups with 120 such docs each at limit 100: every launch hands over 100 candidates of the query -- 300 through the shared
    list, which is sized for them (nothing is lost to its capacity: the batch is not handed back) --, and the 100 lowest ids come back"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2015)
    w, p, hashes, firsts = _crowd(Pair, ctx, rng, 3, 120)
    queries = []
    for i in range(6):
        q = np.concatenate([hashes, _noise(rng, 300)])
        rng.shuffle(q)
        queries.append(q)
    for m in (1, 2):
        got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=100, min_score=m, min_score_pct=0), want=TAKEN | SECOND_TRIP)
        assert all(g == [(firsts[0] + 100 + i, 30) for i in range(100)] for g in got), got[0][:3]
    got, _ = _both(ctx, p, queries, fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=0), want=TAKEN | SECOND_TRIP)
    assert all(len(g) == 360 and all(s == 30 for _, s in g) for g in got), [len(g) for g in got]


# ---- 3. the chained hand-over under low floors ------------------------------------------------------------------------------------------

# candidates of a query per group (tests/test_gpu_groups_wg.py::test_the_chained_hand_over's): three hashes list the same k docs of the
# group's first column, a score of 3 -- above a floor of 2, by the sorted tail
CASES = [(2, 2, 0), (3, 2, 0), (6, 1, 0), (0, 3, 0), (3, 0, 0), (1, 40, 0), (1, 1, 3)]
IN_SLOTS = (0, 3, 4)                # the cases that never leave the queries' own four slots


def _hand(c, j):
    return HAND + 7919 * (3 * c + j)


def _hand_extra(gi):
    return lambda s, ids: [(_hand(c, j), ids[50 * c: 50 * c + k[gi]]) for c, k in enumerate(CASES) for j in range(3) if s == 0 and k[gi]]


def test_the_chained_hand_over_under_low_floors(tiny):
    """2 + 2: the slots fill exactly; 3 + 2: the earlier slots move to the shared list; 6 + 1: the first launch overflowed already; 0 + 3
    (no record of the query in the first group); 3 + 0 (none in the second: the first launch's slots and count stay); 1 + 40: more than
    the LDS buffer's 32 in the later group; 1 + 1 + 3 over three groups.  min_score 2, pct 0, limit 500: every query's docs, each with a
    score of 3.  The shared list was used (bit 1) -- and is not by a batch of 2 + 2, 0 + 3 and 3 + 0 alone"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2020)
    w = wg.World(Pair, ctx)
    firsts = [1]
    _, nxt = w.columns(rng, 3, 600, 40, _hand_extra(0))
    firsts.append(nxt)
    nxt = _more(w, rng, 2, 600, 40, nxt, _hand_extra(1))
    w.finish()
    firsts.append(nxt)
    _more(w, rng, 2, 600, 40, nxt, _hand_extra(2))
    p = _finish(w, 2)
    assert _layout(p) == [(3, 8, 1), (2, 8, 1), (2, 8, 1)], _layout(p)

    def query(c):
        q = np.concatenate([np.array([_hand(c, j) for j in range(3)], dtype=np.uint32), _noise(rng, 47)])
        rng.shuffle(q)
        return q

    def docs(c):
        return sorted(firsts[gi] + 50 * c + i for gi in range(3) for i in range(CASES[c][gi]))

    low = fpx.SearchOptions(max_results=500, min_score=2, min_score_pct=0)
    order = [c for c in range(len(CASES)) for _ in range(3)]
    queries = [query(c) for c in order]
    got, _ = _both(ctx, p, queries, low, want=TAKEN | SECOND_TRIP)
    for c, g in zip(order, got):
        assert sorted(d for d, _ in g) == docs(c) and all(s == 3 for _, s in g), (CASES[c], g[:8])
    order = [c for c in IN_SLOTS for _ in range(4)]
    queries = [query(c) for c in order]
    got, _ = _both(ctx, p, queries, low, want_not=SECOND_TRIP)
    for c, g in zip(order, got):
        assert sorted(d for d, _ in g) == docs(c) and all(s == 3 for _, s in g), (CASES[c], g[:8])


# ---- 4. mixed floors and lengths in one batch -------------------------------------------------------------------------------------------

def test_mixed_floors_and_lengths_in_one_batch(tiny):
    """explicit floors 1, 2, 3 and 50 and the default one; lengths 0, 1, 2, 40, 41 (default floors 2 and 3), 256 and 4096, of a doc of
    each group: the sorted tail and the usual one take turns in every launch's workgroups"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2030)
    w, end0, _ = _two_groups(Pair, ctx, rng, 5, 2, 700, 700, _usual, _usual)
    p = _finish(w, 2)
    assert _layout(p) == [(5, 8, 1), (2, 8, 1)], _layout(p)
    shapes = []
    for doc, items in ((300, w.items[0]), (end0 + 30, w.items[5])):
        own = _rows(items, doc)
        assert len(own) >= 38, len(own)
        shapes += [np.zeros(0, dtype=np.uint32), own[:1], own[:2],
                   np.concatenate([own[:30], _noise(rng, 10)]),
                   np.concatenate([own[:30], _noise(rng, 11)]),
                   np.concatenate([own, _noise(rng, 256 - len(own))]),
                   np.concatenate([own, _noise(rng, QS_MAX_HASHES - len(own))])]
    assert [len(x) for x in shapes[:7]] == [0, 1, 2, 40, 41, 256, 4096]
    floors = [1, 2, 3, 50, None]
    queries, opts = [], []
    for i, q in enumerate(shapes):
        for j in range(2):                                     # (every shape under two of the floors, the pairs rotating)
            queries.append(q)
            opts.append(fpx.SearchOptions(max_results=[100, 1, 3][(i + j) % 3], min_score=floors[(i + 2 * j) % 5], min_score_pct=[0, 10, 100][(i + j) % 3]))
    _both(ctx, p, queries, opts)
    # every shape under every low floor, one floor per batch
    for m in (2, None):
        _both(ctx, p, shapes, fpx.SearchOptions(max_results=100, min_score=m, min_score_pct=0))
    got, _ = _both(ctx, p, shapes, fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0))
    assert got[0] == [] and got[1][0] == (300, 1) and got[5][0][0] == 300 and got[8][0] == (end0 + 30, 1) and got[13][0][0] == end0 + 30, (got[1][:1], got[8][:1])


# ---- 5. a memory segment below both groups ----------------------------------------------------------------------------------------------

def test_a_memory_segment_below_both_groups(tiny):
    """the groups' docs start at 1000; a memory segment holds docs 5 .. 44 -- below every group's gmin: their records wrap in the first
    launch, which alone carries the memory table, and the sorted tail adds THAT group's gmin back -- under the legacy options.  A query
    that finds only a memory doc returns it"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2040)
    w, nxt, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual, _usual, first=1000)
    ids = np.arange(5, 45)
    w.memory(_rand_items(rng, ids, 40), ids)
    p = _finish(w, 2)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)] and p.reader.snapshot.info()["memory"] == 1
    mem = w.items[-1]
    queries = [np.concatenate([_rows(mem, 5), _noise(rng, 360)]), np.concatenate([_rows(mem, 20), _noise(rng, 360)])] + _queries(rng, w, 22)
    got, _ = _both(ctx, p, queries, _legacy(fpx), want_not=TWO_PARTS)
    assert got[0][0][0] == 5 and [d for d, _ in got[1]] == [20], (got[0][:2], got[1])
    assert any(g and 5 <= g[0][0] < 45 for g in got[2:]) and any(g and g[0][0] >= nxt for g in got[2:])
    # a limit that cuts inside the tie at a score of 1: the memory docs' REAL ids are the lowest
    one_each = np.array([int(_rows(mem, d)[d % 7]) for d in ids], dtype=np.uint32)
    both_groups = np.concatenate(w.items[:6])
    queries = [np.concatenate([one_each, _sampled(rng, both_groups, 300), _noise(rng, 60)]) for _ in range(4)] + queries[:8]
    got, _ = _both(ctx, p, queries, fpx.SearchOptions(max_results=20, min_score=1, min_score_pct=0), want_not=TWO_PARTS)
    for g in got[:4]:
        top = [d for d, s in g if s == 1]
        assert len(g) == 20 and top == sorted(top) and top and top[-1] < 45, g


# ---- 6. record counts at the sorted tail's edges, in the second group -------------------------------------------------------------------

@pytest.fixture
def edges(tiny):
    """a first group of 2 columns; the SECOND group has 8: HOT8 has 1000 docs in each of them, HOT1 1000 docs of its column 0, its column 1
    holds 3500 hashes of one doc each, its column 2 three docs with 300 hashes (BIG ..) and two with 260 of those"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2050)
    singles = [SINGLE + 7919 * k for k in range(3500)]
    big = np.array([BIG + k * 7919 for k in range(300)], dtype=np.uint32)

    def extra(s, ids):
        e = [(HOT8, ids[:1000])]
        if s == 0:
            e.append((HOT1, ids[200:1200]))
        if s == 1:
            e += [(h, ids[i % len(ids): i % len(ids) + 1]) for i, h in enumerate(singles)]
        if s == 2:
            e += [(int(h), ids[10:13]) for h in big] + [(int(h), ids[20:22]) for h in big[:260]]
        return e

    w = wg.World(Pair, ctx)
    _, nxt = w.columns(rng, 2, 500, 40, _usual)
    _more(w, rng, 8, 1200, 24, nxt, extra)
    p = _finish(w, 2)
    assert _layout(p) == [(2, 8, 1), (8, 8, 1)], _layout(p)
    return fpx, ctx, rng, w, p, np.array(singles, dtype=np.uint32), big, nxt


def _records(p, q):
    return p.osnap.search(q, 40, 1, 0, with_stats=True)[1].scanned_docs


_exact = functools.partial(wg.exact, _records)


def test_record_counts_at_the_sorted_tails_edges_in_the_second_group(edges):
    """255, 256, 257 and 4097 records (the network's smallest size, and the power of two above 4096) and 8150 (just under the array's
    8192), all of them in the SECOND group and none in the first; a limit of 100 at min_score_pct 0 cuts inside the tie at 1"""
    fpx, ctx, rng, w, p, singles, big, nxt = edges
    sizes = (([], 255), ([], 256), ([], 257), ([HOT1], 4097), ([HOT8], 8150))
    queries = [_exact(p, rng, head, singles, target) for head, target in sizes]
    assert [_records(p, q) for q in queries] == [t for _, t in sizes]
    first = np.concatenate(w.items[:2])
    assert not any(np.isin(q, (first >> wg.U64(32)).astype(np.uint32)).any() for q in queries)       # (nothing in the first group)
    for i in range(7):                                         # (five docs in six of the second group hold HOT8 themselves)
        q = _aimed(rng, w.items[i % 10], 300)
        queries.append(q[(q != HOT8) & (q != HOT1)])
    for opts in (fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0), fpx.SearchOptions(max_results=500, min_score=2, min_score_pct=0), _legacy(fpx)):
        _both(ctx, p, queries, opts)


def test_scores_beyond_the_histograms_last_slot_in_the_second_group(edges):
    """three docs with 300 of the query's hashes and two with 260, in the second group: the sorted tail's histogram has one slot for every
    score from 255 up, so a cut that falls there keeps the slot whole -- k_finish makes the cut; limits inside and outside the two ties,
    and a relative floor above 255"""
    fpx, ctx, rng, w, p, singles, big, nxt = edges
    other = np.concatenate(w.items[:2] + w.items[5:])
    d0 = nxt + 2 * 1200                                        # (the second group's column 2 starts here)
    queries = []
    for i in range(8):
        q = np.concatenate([big if i % 2 == 0 else big[:280], _sampled(rng, other, 400), _noise(rng, 100)])
        q = q[(q != HOT8) & (q != HOT1)]
        rng.shuffle(q)
        queries.append(q)
    sets = [fpx.SearchOptions(max_results=k, min_score=m, min_score_pct=pct)
            for k, m, pct in ((1, 1, 0), (2, 1, 0), (4, 1, 0), (100, 1, 0), (500, 1, 100), (500, 2, 90), (500, 1, 10), (5, 2, 0))]
    got, st = _both(ctx, p, queries, sets)
    assert got[0] == [(d0 + 10, 300)] and got[1] == [(d0 + 10, 280), (d0 + 11, 280)], got[:2]
    assert got[2] == [(d0 + 10, 300), (d0 + 11, 300), (d0 + 12, 300), (d0 + 20, 260)], got[2]
    assert got[4] == [(d0 + 10, 300), (d0 + 11, 300), (d0 + 12, 300)] and len(got[3]) == 100, got[4]
    assert [d for d, _ in got[5]] == [d0 + 10, d0 + 11, d0 + 12, d0 + 20, d0 + 21], got[5]
    for o in sets[:4]:
        _both(ctx, p, queries, o)


# ---- 7. filtered groups: low_wg = 2 under query_wg = 2 ----------------------------------------------------------------------------------

def _filtered(fpx, ctx, p, queries, want):
    """under low_wg = 2, query_wg = 2: taken, bit 8 set; the same world under low_wg = 1: the pipeline -- bits 13, 12 and 6 clear"""
    got, _ = _both(ctx, p, queries, _legacy(fpx), want=want, low_wg=2, also=(("query_wg", 2),))
    _both(ctx, p, queries, fpx.SearchOptions(max_results=7, min_score=1, min_score_pct=0), want=want, low_wg=2, also=(("query_wg", 2),))
    _both(ctx, p, queries, _legacy(fpx), want=GROUP, want_not=GROUPS | LOW | QUERY_WG, low_wg=1, also=(("query_wg", 2),))
    return got


def test_a_dead_set_in_the_first_group_only(tiny):
    """the second group's newest column writes doc 17 of the first group again: group 0 has a dead set, group 1 none -- the first launch is
    k_search_low_filt, the second the unfiltered k_search_low_next"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2060)
    w = wg.World(Pair, ctx, snapshot_query_wg=2)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    _more(w, rng, 2, 600, 40, nxt, _usual, again=(17,))
    p = _finish(w, 2)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)], _layout(p)
    queries = [np.concatenate([_rows(w.items[0], 17), _noise(rng, 360)])] + _queries(rng, w, 23)
    got = _filtered(fpx, ctx, p, queries, TAKEN | FILTERED)
    assert got[0][0][0] == 17 and [d for d, _ in got[0]].count(17) == 1, got[0][:3]


def test_a_dead_set_in_the_second_group_only(tiny):
    """the second group's newest column writes a doc of the second group's OWN first column again: group 1 has a dead set, group 0 none --
    the first launch is the unfiltered k_search_low, the second the filtered k_search_low_next"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2065)
    w = wg.World(Pair, ctx, snapshot_query_wg=2)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    doc = nxt + 16
    _more(w, rng, 3, 600, 40, nxt, _usual, again=(doc,))
    p = _finish(w, 2)
    assert _layout(p) == [(4, 8, 1), (3, 8, 1)], _layout(p)
    queries = [np.concatenate([_rows(w.items[4], doc), _noise(rng, 360)])] + _queries(rng, w, 23)
    got = _filtered(fpx, ctx, p, queries, TAKEN | FILTERED)
    assert got[0][0][0] == doc and [d for d, _ in got[0]].count(doc) == 1, got[0][:3]


def test_two_columns_merged_away_from_the_first_group(tiny):
    """the first group's two oldest columns are merged into a segment of its own (no regroup): the group keeps two columns outside the
    snapshot -- `active` is not all --, the merged segment is part 1 of a snapshot made under groups_wg = 2, query_wg = 2, both groups
    part 0: bits 13, 12, 8 and 7"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2070)
    w = wg.World(Pair, ctx, snapshot_query_wg=2)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    _more(w, rng, 2, 600, 40, nxt, _usual)
    p = w.finish()
    merged = p.reader.snapshot.merge(p.gpu_segs[0:2], 512)
    want = p.osnap.merge(p.orc_file[0:2])
    wb, wi = oracle.build_blocks(want["items"], want["min_doc_id"], 512)
    q = wg.World(Pair, ctx, snapshot_query_wg=2)
    q.items, q.commit = list(w.items), 10
    q.p.gpu_segs = [merged] + p.gpu_segs[2:]
    q.p.orc_file = [oracle.file_segment(wb, 512, wi, want["min_doc_id"], want["max_doc_id"], want["commit_id"], want["doc_ids"], want["doc_alive"])] + p.orc_file[2:]
    _finish(q, 2)
    assert q.p.reader.snapshot.info()["groups"] == 2
    queries = [np.concatenate([_rows(w.items[0], 17), _noise(rng, 360)])] + _queries(rng, w, 23)
    got = _filtered(fpx, ctx, q.p, queries, TAKEN | FILTERED | TWO_PARTS)
    assert got[0][0][0] == 17 and [d for d, _ in got[0]].count(17) == 1, got[0][:3]       # (found in the merged segment, once)


# ---- 8. two parts -----------------------------------------------------------------------------------------------------------------------

def test_two_parts(tiny):
    """two groups, a checkpoint in blocks and a memory segment under the legacy options.  The snapshot made under groups_wg = 2: part 0 is
    BOTH groups (and the memory segment), by k_search_low and k_search_low_next, part 1 the checkpoint, by the pipeline: bits 13, 12 and
    7; best docs from all four places"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2080)
    w, end0, nxt = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual, _usual)
    ids = np.arange(nxt, nxt + 500)
    w.file(_rand_items(rng, ids, 40, [(SHARED, ids[:7])]), ids, form="blocks")
    ids = np.arange(nxt + 500, nxt + 540)
    w.memory(_rand_items(rng, ids, 40), ids)
    p = _finish(w, 2)
    info = p.reader.snapshot.info()
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)] and info["groups"] == 2 and info["memory"] == 1 and not p.gpu_segs[6].grouped, info
    queries = _queries(rng, w, 32)
    got, _ = _both(ctx, p, queries, _legacy(fpx), want=TAKEN | TWO_PARTS)
    assert len({(g[0][0] >= end0) + (g[0][0] >= nxt) + (g[0][0] >= nxt + 500) for g in got if g}) == 4      # (both groups, the checkpoint, the memory segment)
    _both(ctx, p, queries, fpx.SearchOptions(max_results=7, min_score=1, min_score_pct=0), want=TAKEN | TWO_PARTS)


# ---- 9. a hand-back from the second launch ----------------------------------------------------------------------------------------------

def test_records_beyond_the_array_in_the_second_group_are_handed_back(tiny):
    """five hashes with 1000 docs each in both columns of the SECOND group: 10 000 hit records there, over the array's 8192, nothing in the
    first -- the existing hand-back, under the legacy options.  The batch comes back right, by the pipeline; the snapshot's next batch
    stays there (the back-off); a fresh snapshot is taken again"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2090)
    hot = np.array([HOTB + 7919 * k for k in range(5)], dtype=np.uint32)
    w, _, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 1200, _usual, lambda s, ids: [(int(h), ids[:1000]) for h in hot])
    p = _finish(w, 2)
    opts = _legacy(fpx)
    plain = [q[~np.isin(q, hot)] for q in _queries(rng, w, 12)]      # (a doc of the second group's first thousand has the five among its own)
    heavy = list(plain)
    heavy[5] = np.concatenate([hot, _noise(rng, 60)])
    assert sum(s for _, s in p.osnap.search(heavy[5], 1 << 20, 1, 0)) > QS_REC_CAP
    got, _ = _both(ctx, p, plain, opts)
    ctx.set_option("groups_wg", 2)
    ctx.set_option("low_wg", 1)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & (GROUPS | LOW | QUERY_WG) and st_h.path_flags & GROUP, f"not handed back ({st_h.path_flags})"
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, opts.max_results, opts.min_score, opts.min_score_pct)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernels)
        assert not st_n.path_flags & (GROUPS | LOW | QUERY_WG) and got_n == got, st_n.path_flags
    finally:
        ctx.set_option("groups_wg", -1)
        ctx.set_option("low_wg", -1)
    p = _finish(w, 2)                                          # a fresh snapshot of the same segments
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


# ---- 10. many queries from host memory, and a deadline ----------------------------------------------------------------------------------

def test_a_batch_uploaded_in_pieces_and_a_deadline(tiny):
    """2400 queries of 450 hashes from host memory, every third one with the legacy options: more than the chip's 1024 workgroups (every
    launch hands its queries out through a counter of its own) and large enough to be uploaded in pieces -- the groups are walked piece
    by piece.  == the batch under 0.  With a deadline of 1 ms the call is a timeout or complete and right, nothing else; the next call
    without a deadline is right"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2100)
    w, _, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual, _usual)
    p = _finish(w, 2)
    queries = _queries(rng, w, 24, qlen=450) * 100
    opts = [_legacy(fpx) if i % 3 == 0 else fpx.http_options() for i in range(len(queries))]
    assert sum(len(q) for q in queries) >= 1 << 20
    ctx.set_option("low_wg", 1)
    ctx.set_option("groups_wg", 0)
    try:
        want, st0 = p.reader.search_batch(queries, opts)
        assert not st0.path_flags & (GROUPS | LOW)
        ctx.set_option("groups_wg", 2)
        got, st = p.reader.search_batch(queries, opts)
        assert st.path_flags & TAKEN == TAKEN, st.path_flags
        assert got == want and wg.figures(st) == wg.figures(st0), (wg.figures(st), wg.figures(st0))
        try:
            timed, _ = p.reader.search_batch(queries, opts, timeout_ms=1)
            assert timed == want
        except fpx.SearchTimeout as e:
            assert e.status == -2
        again, st2 = p.reader.search_batch(queries, opts)
        assert again == want and st2.path_flags & TAKEN == TAKEN, st2.path_flags
    finally:
        ctx.set_option("groups_wg", -1)
        ctx.set_option("low_wg", -1)


# ---- 11. what stays off -----------------------------------------------------------------------------------------------------------------

def test_without_low_wg_a_legacy_query_keeps_the_batch_off(tiny):
    """groups_wg = 2 with low_wg = 0 and one legacy query in the batch: the pipeline's"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2110)
    w, _, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual, _usual)
    p = _finish(w, 2)
    queries = _queries(rng, w, 12)
    opts = [fpx.http_options()] * 12
    opts[3] = _legacy(fpx)
    _both(ctx, p, queries, opts, want=GROUP, want_not=GROUPS | QUERY_WG | LOW, low_wg=0)
    _both(ctx, p, queries, opts)                               # (with low_wg = 1: taken)


def test_a_batch_without_a_low_floor_is_taken_as_under_1(tiny):
    """groups_wg = 2 with no low floor in the batch: k_search_query and k_search_next exactly as under 1 -- bit 12 clear, results and
    figures equal to groups_wg = 1's"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2120)
    w, _, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual, _usual)
    p = _finish(w, 2)
    queries = _queries(rng, w, 16)
    for low_wg in (0, 1):
        got, st = _both(ctx, p, queries, fpx.http_options(), want=GROUPS | QUERY_WG | GROUP, want_not=LOW, low_wg=low_wg)
    ctx.set_option("low_wg", 1)
    try:
        ctx.set_option("groups_wg", 1)
        g1, s1, qb1, qd1 = p.reader.search_batch_stats(queries, fpx.http_options())
        ctx.set_option("groups_wg", 2)
        g2, s2, qb2, qd2 = p.reader.search_batch_stats(queries, fpx.http_options())
    finally:
        ctx.set_option("groups_wg", -1)
        ctx.set_option("low_wg", -1)
    assert s1.path_flags == s2.path_flags and s2.path_flags & (GROUPS | QUERY_WG | LOW) == GROUPS | QUERY_WG, (s1.path_flags, s2.path_flags)
    assert g1 == g2 == got and wg.figures(s1) == wg.figures(s2)
    assert [int(x) for x in qb1] == [int(x) for x in qb2] and [int(x) for x in qd1] == [int(x) for x in qd2]


def test_a_group_in_directory_and_words_form_among_them(tiny):
    """the second group in directory + words form: not walked this way -- the packed group alone is part 0 of the snapshot's two parts, by
    k_search_low (bit 12 without bit 13)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2130)
    w = wg.World(Pair, ctx)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    ctx.set_option("group_packed", 0)
    _more(w, rng, 2, 600, 40, nxt, _usual)
    p = _finish(w, 2)
    assert _layout(p) == [(4, 8, 1), (2, 8, 0)], _layout(p)
    wg.both(ctx, p, _queries(rng, w, 16), _legacy(fpx), "groups_wg", 2, clear=GROUPS, want=GROUP, want_not=GROUPS, also=(("low_wg", 1),))
