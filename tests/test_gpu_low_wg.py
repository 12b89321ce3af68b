"""k_search_low (csrc/fpx_qsearch.hpp, option low_wg = 1): a batch with queries whose score floor is 1 or 2 -- the legacy protocol's
min_score 1, the default floor of a query of 40 hashes or fewer -- stays on the query-per-workgroup path of a packed, unfiltered group
instead of going to the pipeline.  Such a query's records are sorted in LDS, a doc's score is the length of its run, the floor is raised
by the query's best score and only what finish can return -- the top max_results in (score descending, id ascending) order -- is handed
over.  fpx_stats.path_flags bit 12 (4096) says that a batch, or its part 0, ran the kernel; bits 6 and 2 are set with it.

Every case goes through Pair.check under the option (results and every query's scanned blocks / docs == the oracle's) with the path bits
asserted, and is then run again under the option and under low_wg = 0 and compared byte for byte: results, scanned_blocks, scanned_docs,
probes, hits, algorithmic_bytes, per-query blocks / docs and the growth of the context's scan histograms (nothing unbucketed).  The
groups are tiny (group_packed = 1, FPX_DIRECT_MIN_ITEMS = 0), one at a time: each case is the smallest shape that reaches its branch."""
import functools

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import (FILTERED, GROUP, LOW, QS_MAX_HASHES, QUERY_WG, SECOND_TRIP, TWO_PARTS, U64, HOT8, HOT1,
                        aimed as _aimed, figures as _figures, legacy as _legacy, noise as _noise, rand_items as _rand_items, rows as _rows,
                        sampled as _sampled)

pytestmark = pytest.mark.gpu

SHARED, DOUBLE, CROWD, SINGLE = 0x2BADF00D, 0x37770000, 0x51515151, 0x70000000
OPTIONS = ("low_wg", "hot_wg", "query_wg", "direct_min_items")
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


def World(Pair, ctx):
    """a Pair whose file segments meet in ONE packed group; checkpoints, a merged segment and memory segments next to it"""
    return wg.World(Pair, ctx, packed=1)


def _both(ctx, p, queries, opts, want=LOW | QUERY_WG | GROUP, want_not=0, also=()):
    """Pair.check under low_wg = 1 with the path bits asserted, then the batch under the option and under 0, everything equal.  Under 0 a
    batch with a low floor is the pipeline's, as before: bit 6 clear as well"""
    return wg.both(ctx, p, queries, opts, "low_wg", 1, clear=LOW | (QUERY_WG if want & LOW else 0), want=want, want_not=want_not, also=also,
                   compare=wg.WITH_BYTES)      # (algorithmic_bytes too)


# ---- 1. the legacy protocol -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_legacy_options(tiny, cols):
    """5 columns (lines of 8 hash values) and 9 (lines of 4); 24 queries of 1000 hashes aimed at their own docs: the best score is at least
    30, so the floor is raised.  The first test of the file: on the parent set_option("low_wg", ...) is refused"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1500 + cols)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, cols, 1500 if cols == 5 else 800, 64, _usual)
    queries = [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE][: i % 3]) for i in range(24)]
    got, st = _both(ctx, p, queries, _legacy(fpx))
    assert all(g and g[0][1] >= 30 for g in got), [g[:1] for g in got]
    # the option is off by default
    _, st_d = p.reader.search_batch(queries, _legacy(fpx))
    assert not st_d.path_flags & (LOW | QUERY_WG) and st_d.path_flags & GROUP, st_d.path_flags


# ---- 2. nothing raises the floor ------------------------------------------------------------------------------------------------

@pytest.fixture
def crowd(tiny):
    """200 docs of column 0 share thirty hashes: a tie at a score of 30"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1510)
    w = World(Pair, ctx)
    hashes = np.array([CROWD + k * 7919 for k in range(30)], dtype=np.uint32)
    p, _ = w.columns(rng, 4, 1200, 40, lambda s, ids: [(int(c), ids[100:300]) for c in hashes] if s == 0 else [])
    return fpx, ctx, rng, w, p, hashes


def test_nothing_raises_the_floor(crowd):
    """min_score_pct 0, min_score 1 and 2, limits 1, 7, 100 and 500: the tie of 200 docs at 30 straddles the limits 100 and 7, the
    thousands of docs at a score of 1 that the sampled hashes give are the tie at the cut for limit 500 -- the top-K cut does all the work"""
    fpx, ctx, rng, w, p, hashes = crowd
    allitems = np.concatenate(w.items[1:])                    # (the sampled hashes stay off the crowd's column: its tie stays a tie)
    sets = [fpx.SearchOptions(max_results=k, min_score=m, min_score_pct=0) for m in (1, 2) for k in (1, 7, 100, 500)]
    queries, opts = [], []
    for i in range(16):
        few = i >= 8
        q = np.concatenate([hashes[:10] if few else hashes, _sampled(rng, allitems, 3000 if few else 1500), _noise(rng, 200)])
        rng.shuffle(q)
        queries.append(q)
        opts.append(sets[i % 8])
    got, st = _both(ctx, p, queries, opts, want=LOW | QUERY_WG | GROUP | SECOND_TRIP)
    full = 0
    for q, o, g in zip(queries, opts, got):
        want = p.osnap.search(q, o.max_results, o.min_score, o.min_score_pct)
        if len(want) == o.max_results:
            assert len(g) == o.max_results, (len(g), o)
            full += 1
    assert full >= 12, full
    assert [s for _, s in got[2]] == [30] * 100 and [d for d, _ in got[2]] == list(range(101, 201)), got[2][:3]      # (min_score 1, limit 100, thirty hashes)
    assert len(got[3]) == 500 and got[3][200][1] < 30 and got[3][-1][1] == 1, got[3][198:203]      # (... limit 500: the cut is inside the tie at 1)


# ---- 3. mixed floors in one batch -----------------------------------------------------------------------------------------------

@pytest.fixture
def shapes(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1520)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 5, 1500, 64, lambda s, ids: _usual(s, ids) + [(0, ids[:2]), (0xFFFFFFFF, ids[5:8])][: 2 if s % 2 == 0 else 0])
    return fpx, ctx, rng, w, p


def test_mixed_floors_in_one_batch(shapes):
    """explicit floors 1, 2, 3 and 50 and the default one; lengths 0, 1, 2, 40, 41 (default floors 2 and 3), 256, 257 and 4096;
    duplicates inside a query; the hashes 0 and 0xFFFFFFFF"""
    fpx, ctx, rng, w, p = shapes
    own = _rows(w.items[0], 300)
    shapes_ = [np.zeros(0, dtype=np.uint32),
               own[:1],
               own[:2],
               np.concatenate([own[:30], _noise(rng, 10)]),
               np.concatenate([own[:30], _noise(rng, 11)]),
               np.concatenate([own, _noise(rng, 256 - len(own))]),
               np.concatenate([own, _noise(rng, 257 - len(own))]),
               np.concatenate([own, _noise(rng, QS_MAX_HASHES - len(own))]),
               np.full(500, int(own[0]), dtype=np.uint32),
               np.concatenate([own, own, own[:7], np.array([SHARED, SHARED, DOUBLE], dtype=np.uint32)]),
               np.array([0, 0xFFFFFFFF, 5, 6, 7], dtype=np.uint32),
               np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32),
               _aimed(rng, w.items[3], 1000, [0, 0xFFFFFFFF, SHARED])]
    assert [len(x) for x in shapes_[:8]] == [0, 1, 2, 40, 41, 256, 257, 4096]
    floors = [1, 2, 3, 50, None]
    queries, opts = [], []
    for i, q in enumerate(shapes_):
        for j in range(2):                                     # (every shape under two of the floors, the pairs rotating)
            queries.append(q)
            opts.append(fpx.SearchOptions(max_results=[100, 1, 3][(i + j) % 3], min_score=floors[(i + 2 * j) % 5], min_score_pct=[0, 10, 100][(i + j) % 3]))
    got, st = _both(ctx, p, queries, opts)
    # every shape under every floor, one floor per batch
    for m in (1, 2, None):
        _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=m, min_score_pct=0))
    got, _ = _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0))
    assert got[0] == [] and got[1][0] == (300, 1) and got[5][0] == (300, len(own)) and got[9][0] == (300, len(own))
    # a batch in which NO query is low: k_search_query, whatever the option says
    high = [q for q in shapes_ if len(q) > 40]
    _both(ctx, p, high, fpx.http_options(), want=QUERY_WG | GROUP, want_not=LOW)
    _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0), want=QUERY_WG | GROUP, want_not=LOW)


# ---- 4. memory segments, ids across gmin ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [100_000, (1 << 32) - 4 * 1500])
def test_memory_segments_with_ids_below_the_groups_first(tiny, first):
    """the group's columns start at doc 100 000 (or end at 0xFFFFFFFF); memory segments hold docs 5 .. 60 -- below gmin: their records
    wrap -- and (the first world) docs above the group.  The order at the cut is the order of REAL ids: with min_score_pct 0 and a limit
    that cuts inside the tie at a score of 1, the memory docs below gmin are the first taken"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1530 + first % 7)
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 4, 1500, 48, _usual, first=first)
    below = np.arange(5, 61)
    w.memory(_rand_items(rng, below[:30], 48, [(SHARED, below[:3])]), below[:30])
    w.memory(_rand_items(rng, below[30:], 48), below[30:])
    if nxt < (1 << 32):
        above = np.arange(nxt, nxt + 60)
        w.memory(_rand_items(rng, above, 48, [(SHARED, above[:3])]), above)
    p = w.finish()
    assert p.reader.snapshot.info()["memory"] == (3 if nxt < (1 << 32) else 2)
    group_items, mem_items = np.concatenate(w.items[:4]), np.concatenate(w.items[4:6])
    one_each = np.array([int(_rows(mem_items, d)[d % 7]) for d in below], dtype=np.uint32)      # a hash of every memory doc below gmin
    queries = [np.concatenate([one_each, _sampled(rng, group_items, 300), _noise(rng, 100)]) for _ in range(6)]
    queries += [_aimed(rng, w.items[i % len(w.items)], 600, [SHARED, DOUBLE]) for i in range(12)]
    got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=20, min_score=1, min_score_pct=0))
    for g in got[:6]:
        top = [d for d, s in g if s == 1]
        assert len(g) == 20 and top == sorted(top) and top and top[-1] <= 60, g
    _both(ctx, p, queries, _legacy(fpx))
    got, _ = _both(ctx, p, queries, fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=0))
    assert {d for d, _ in got[0]} >= set(int(d) for d in below)


# ---- 5. more queries than workgroups --------------------------------------------------------------------------------------------

def test_more_queries_than_workgroups(shapes):
    """2100 queries of 8 hashes: more than the 1024 workgroups an MI355X holds.  Default options (a floor of 1) alternate with a floor of
    3: the sorted tail and the usual one take turns in a workgroup, and nothing of one query's array, flags or histogram reaches the next"""
    fpx, ctx, rng, w, p = shapes
    queries, opts = [], []
    for i in range(2100):
        doc = 1 + (i * 37) % 7500
        q = np.concatenate([_rows(w.items[(doc - 1) // 1500], doc)[: 3 + i % 5], np.array([SHARED, 0][: i % 3], dtype=np.uint32)])
        queries.append(np.concatenate([q, _noise(rng, 8 - len(q))]) if len(q) < 8 else q[:8])
        opts.append(fpx.http_options() if i % 2 == 0 or i % 7 == 0 else fpx.SearchOptions(max_results=10, min_score=3, min_score_pct=0))
    got, st = _both(ctx, p, queries, opts)
    assert sum(1 for g in got if g) > 1500


# ---- 6. record counts at the array's edges --------------------------------------------------------------------------------------

@pytest.fixture
def edges(tiny):
    """8 columns; HOT8 has 1000 docs in each of them, HOT1 1000 docs in column 0; column 1 holds 3500 hashes of one doc each"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1540)
    w = World(Pair, ctx)
    singles = [SINGLE + 7919 * k for k in range(3500)]

    def extra(s, ids):
        e = [(HOT8, ids[:1000])]
        if s == 0:
            e.append((HOT1, ids[200:1200]))
        if s == 1:
            e += [(h, ids[i % len(ids): i % len(ids) + 1]) for i, h in enumerate(singles)]
        return e

    p, _ = w.columns(rng, 8, 1200, 24, extra)
    return fpx, ctx, rng, w, p, np.array(singles, dtype=np.uint32)


def _records(p, q):
    return p.osnap.search(q, 40, 1, 0, with_stats=True)[1].scanned_docs


_exact = functools.partial(wg.exact, _records)


def test_record_counts_at_the_arrays_edges(edges):
    """255, 256, 257 and 4097 records (the network's smallest size, and the power of two above 4096), 8150 (just under the array's 8192),
    and a size for each network in between; a limit of 100 at min_score_pct 0 cuts inside the tie at 1"""
    fpx, ctx, rng, w, p, singles = edges
    sizes = (([], 255), ([], 256), ([], 257), ([HOT1], 4097), ([HOT8], 8150), ([], 600), ([], 1500), ([], 3000))      # (the last three: the networks of 1024, 2048 and 4096)
    queries = [_exact(p, rng, head, singles, target) for head, target in sizes]
    assert [_records(p, q) for q in queries] == [t for _, t in sizes]
    for i in range(7):                                         # (five docs in six hold HOT8 themselves)
        q = _aimed(rng, w.items[i % 8], 300)
        queries.append(q[(q != HOT8) & (q != HOT1)])
    for opts in (fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0), fpx.SearchOptions(max_results=500, min_score=2, min_score_pct=0), _legacy(fpx)):
        got, st = _both(ctx, p, queries, opts)


def test_records_beyond_the_array_are_handed_back(edges):
    """HOT8 and a few hundred more: over 8192 records.  The batch is the pipeline's (bit 12 clear), so is the next one on that snapshot
    (the back-off); a fresh snapshot takes the kernel again"""
    fpx, ctx, rng, w, p, singles = edges
    plain = [_aimed(rng, w.items[i % 8], 300) for i in range(12)]
    plain = [q[(q != HOT8) & (q != HOT1)] for q in plain]
    heavy = list(plain)
    heavy[5] = np.concatenate([[HOT8], singles[:300]]).astype(np.uint32)
    assert _records(p, heavy[5]) == 8300
    opts = fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0)
    got, st = _both(ctx, p, plain, opts)
    ctx.set_option("low_wg", 1)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & (LOW | QUERY_WG) and st_h.path_flags & GROUP, f"8300 records fit 8192? ({st_h.path_flags})"
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, 100, 1, 0)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernel)
        assert not st_n.path_flags & (LOW | QUERY_WG) and got_n == got, st_n.path_flags
        ctx.set_option("low_wg", 0)
        got_p, st_p = p.reader.search_batch(heavy, opts)
        assert got_p == got_h and _figures(st_p) == _figures(st_h)
    finally:
        ctx.set_option("low_wg", -1)
    p.finish()                                                 # a fresh snapshot of the same segments
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


# ---- 7. crowded hand-over -------------------------------------------------------------------------------------------------------

def test_crowded_queries_take_the_shared_list(crowd):
    """200 docs at a score of 26 .. 30 under the legacy options and under a limit of 100: more candidates than a query's four slots and
    than the 32 of its LDS buffer -- the shared list and the second finish (path_flags bit 1) with bit 12"""
    fpx, ctx, rng, w, p, hashes = crowd
    queries = []
    for i in range(12):
        q = np.concatenate([hashes[: 30 if i % 3 == 0 else 26 + i % 4], _noise(rng, 900)])
        rng.shuffle(q)
        queries.append(q)
    got, st = _both(ctx, p, queries, _legacy(fpx), want=LOW | QUERY_WG | GROUP | SECOND_TRIP)
    assert len(got[0]) == 200
    got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=100, min_score=2, min_score_pct=10), want=LOW | QUERY_WG | GROUP | SECOND_TRIP)
    assert len(got[0]) == 100 and [d for d, _ in got[0]] == list(range(101, 201))


def test_scores_beyond_the_histograms_last_slot(tiny):
    """three docs with 300 of the query's hashes and two with 260: the kernel's histogram has one slot for every score from 255 up, so a
    cut that falls there keeps the slot whole -- k_finish makes the cut; limits inside and outside the two ties, and a relative floor
    above 255"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1555)
    w = World(Pair, ctx)
    big = np.array([0x61000000 + k * 7919 for k in range(300)], dtype=np.uint32)
    p, _ = w.columns(rng, 4, 1200, 40, lambda s, ids: ([(int(h), ids[10:13]) for h in big] + [(int(h), ids[20:22]) for h in big[:260]]) if s == 0 else [])
    other = np.concatenate(w.items[1:])
    queries = []
    for i in range(8):
        q = np.concatenate([big if i % 2 == 0 else big[:280], _sampled(rng, other, 500), _noise(rng, 100)])
        rng.shuffle(q)
        queries.append(q)
    sets = [fpx.SearchOptions(max_results=k, min_score=m, min_score_pct=pct)
            for k, m, pct in ((1, 1, 0), (2, 1, 0), (4, 1, 0), (100, 1, 0), (500, 1, 100), (500, 2, 90), (500, 1, 10), (5, 2, 0))]
    got, st = _both(ctx, p, queries, sets)
    assert got[0] == [(11, 300)] and got[1] == [(11, 280), (12, 280)] and got[2] == [(11, 300), (12, 300), (13, 300), (21, 260)], got[:3]
    assert got[4] == [(11, 300), (12, 300), (13, 300)] and len(got[3]) == 100 and [d for d, _ in got[5]] == [11, 12, 13, 21, 22], (got[4], got[5])
    for o in sets[:4]:
        _both(ctx, p, queries, o)


# ---- 8. two parts ---------------------------------------------------------------------------------------------------------------

def test_two_parts(tiny):
    """a group of 5 columns; next to it two checkpoints in blocks, a merged segment direct-addressed alone and two memory segments: part 0
    -- the group and the memory segments -- by k_search_low, part 1 by the pipeline, k_merge unchanged"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1560)
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 5, 1500, 64, _usual)
    bounds = [(1, nxt)]
    for s in range(2):
        ids = np.arange(nxt, nxt + 800)
        w.file(_rand_items(rng, ids, 64, [(SHARED, ids[:7])]), ids, form="blocks")
        nxt += 800
    bounds.append((bounds[-1][1], nxt))
    ids = np.arange(nxt, nxt + 2000)
    w.file(_rand_items(rng, ids, 64, [(SHARED, ids[:70])]), ids, form="alone")
    nxt += 2000
    bounds.append((bounds[-1][1], nxt))
    for m in range(2):
        ids = np.arange(nxt, nxt + 60)
        w.memory(_rand_items(rng, ids, 64, [(SHARED, ids[:3])]), ids)
        nxt += 60
    bounds.append((bounds[-1][1], nxt))
    p = w.finish()
    assert not any(g.grouped for g in p.gpu_segs[5:8]) and bool(p.gpu_segs[7].direct) and not p.gpu_segs[5].direct, [g.layout_reason for g in p.gpu_segs]
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(40)]      # (a query in ten aims at each addition)
    got, st = _both(ctx, p, queries, _legacy(fpx), want=LOW | QUERY_WG | GROUP | TWO_PARTS)
    found_in = [sum(1 for g in got if g and lo <= g[0][0] < hi) for lo, hi in bounds]
    assert all(n >= 3 for n in found_in), found_in            # the group, the checkpoints, the merged one, the memory segments
    _both(ctx, p, queries, fpx.SearchOptions(max_results=7, min_score=1, min_score_pct=0), want=LOW | QUERY_WG | GROUP | TWO_PARTS)
    # resident in HBM: the same path, the same answers
    ctx.set_option("low_wg", 1)
    try:
        want, _ = p.reader.search_batch(queries, _legacy(fpx))
        qb = fpx.QueryBatch(ctx, queries=queries, options=_legacy(fpx))
        o, n, st_r = fpx.search_resident(p.reader, qb)
        qb.release()
        assert st_r.path_flags & (LOW | QUERY_WG | TWO_PARTS) == LOW | QUERY_WG | TWO_PARTS, st_r.path_flags
        assert fpx.results_to_lists(o, n) == want
    finally:
        ctx.set_option("low_wg", -1)


# ---- 9. not taken ---------------------------------------------------------------------------------------------------------------

def test_a_filtered_group_with_low_floors_is_the_pipelines(tiny):
    """the newest column writes a doc of column 0 again: under query_wg = 2 the group is k_search_query's filtered form for floors above
    2, and the pipeline's for the legacy options -- bits 12 and 8 clear"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1570)
    w = World(Pair, ctx)
    per = 1500
    for s in range(5):
        ids = list(range(1 + s * per, 1 + (s + 1) * per))
        items = _rand_items(rng, ids, 64, _usual(s, np.array(ids)))
        if s == 4:
            src = w.items[0]
            items = np.unique(np.concatenate([items, src[(src & U64(0xFFFFFFFF)) == U64(17)]]))
            ids.append(17)
        w.file(items, sorted(ids))
    p = w.finish()
    assert all(g.grouped for g in p.gpu_segs), [g.layout_reason for g in p.gpu_segs]
    queries = [_aimed(rng, w.items[i % 5], 600, [SHARED]) for i in range(8)]
    _both(ctx, p, queries, _legacy(fpx), want=GROUP, want_not=LOW | FILTERED | QUERY_WG, also=(("query_wg", 2),))
    _both(ctx, p, queries, fpx.http_options(), want=GROUP | QUERY_WG | FILTERED, want_not=LOW, also=(("query_wg", 2),))


def test_batches_the_kernel_does_not_take(shapes):
    fpx, ctx, rng, w, p = shapes
    plain = [_aimed(rng, w.items[i % 5], 600, [SHARED]) for i in range(8)]
    longer = plain[:3] + [np.concatenate([_noise(rng, QS_MAX_HASHES), _rows(w.items[0], 9)[:1]])]
    assert len(longer[3]) == QS_MAX_HASHES + 1
    _both(ctx, p, longer, _legacy(fpx), want=GROUP, want_not=LOW | QUERY_WG)
    _both(ctx, p, plain, _legacy(fpx))                        # (the same batch without the long query: taken)
    # a batch of one (the single query's own path, whatever the option says)
    _both(ctx, p, plain[:1], _legacy(fpx), want=0, want_not=LOW | QUERY_WG)
