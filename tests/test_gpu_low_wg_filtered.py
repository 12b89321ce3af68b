"""k_search_low_filt (csrc/fpx_qsearch.hpp, option low_wg = 2 under query_wg = 2): a batch with queries whose score floor is 1 or 2 -- the
legacy protocol's min_score 1, the default floor of a query of 40 hashes or fewer -- stays on the query-per-workgroup path of a packed
group that is FILTERED: superseded docs (a re-insert, a delete) and/or columns outside the snapshot (a merge without regroup).  The
filtered walk drops a superseded doc where it would be emitted, so the record array holds live docs only and the sorted tail of
k_search_low takes it as it is.  fpx_stats.path_flags: bit 12 (4096) the sorted tail's kernel, bit 8 (256) the filtered form, bit 6 (64)
a query per workgroup, bit 2 (4) a group, bit 7 (128) two parts.

Every case goes through Pair.check under query_wg = 2, low_wg = 2 (results and every query's scanned blocks / docs == the oracle's) with
the path bits asserted, and is then run again under low_wg = 2 and under low_wg = 0 and compared byte for byte: results, scanned_blocks,
scanned_docs, probes, hits, algorithmic_bytes, per-query blocks / docs and the growth of the context's scan histograms (nothing
unbucketed).  The groups are tiny (group_packed = 1, FPX_DIRECT_MIN_ITEMS = 0), one at a time: each case is the smallest shape that
reaches its branch.  The harness is wg_harness.py's, with this file's defaults below."""
import functools

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import (FILTERED, GROUP, LOW, QS_MAX_HASHES, QS_TASKS_FILT, QUERY_WG, TWO_PARTS, U64, HOT8, HOT1,
                        aimed as _aimed, figures as _figures, legacy as _legacy, noise as _noise, post as _post, rand_items as _rand_items,
                        rows as _rows, sampled as _sampled)

pytestmark = pytest.mark.gpu

SHARED, DOUBLE, CROWD, SINGLE, LISTS = 0x2BADF00D, 0x37770000, 0x51515151, 0x70000000, 0x19000000
TAKEN = LOW | FILTERED | QUERY_WG | GROUP
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
    """a Pair whose file segments meet in ONE packed group; checkpoints, a merged segment and memory segments next to it.  Snapshots are
    made under query_wg = 2: a filtered group may be part 0 of a snapshot in two parts"""
    return wg.World(Pair, ctx, packed=1, snapshot_query_wg=2)


def _both(ctx, p, queries, opts, want=TAKEN, want_not=0, query_wg=2):
    """Pair.check under query_wg = 2, low_wg = 2 with the path bits asserted, then the batch under low_wg 2 and under 0, everything equal.
    Under 0 a batch with a low floor is the pipeline's, as before: bit 6 clear as well"""
    return wg.both(ctx, p, queries, opts, "low_wg", 2, clear=LOW | (QUERY_WG if want & LOW else 0), want=want, want_not=want_not,
                   also=(("query_wg", query_wg),), compare=wg.WITH_BYTES)      # (algorithmic_bytes too)


# ---- 1. the legacy protocol on a group with a superseded doc -------------------------------------------------------------------------

def test_legacy_options_on_a_filtered_group(tiny):
    """Five columns, the newest writes doc 17 of column 0 again; 24 queries of 1000 hashes aimed at their own docs under the legacy
    options: bits 12, 8, 6 and 2.  The first test of the file, and the one that FAILS ON THE PARENT: there set_option("low_wg", 2) is
    accepted (only a minimum is checked) but the value is compared == 1, so the batch is the pipeline's and the path-bit assertion fails
    (confirmed once with the parent commit's library: path_flags 4 -- the group, by the pipeline --, AssertionError (4, 4420, 0))"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1600)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 5, 1500, 64, _usual, again={17: None})
    queries = [_aimed(rng, w.items[i % 5], 1000, [SHARED, DOUBLE][: i % 3]) for i in range(23)]
    queries.append(np.concatenate([_rows(w.items[0], 17), _noise(rng, 900)]))      # (the doc written again: found once, in the newest column)
    got, st = _both(ctx, p, queries, _legacy(fpx))
    assert all(g and g[0][1] >= 30 for g in got), [g[:1] for g in got]
    assert got[23][0][0] == 17 and [d for d, _ in got[23]].count(17) == 1, got[23][:3]
    # the option is off by default: the pipeline, under query_wg 2 as well
    ctx.set_option("query_wg", 2)
    try:
        _, st_d = p.reader.search_batch(queries, _legacy(fpx))
    finally:
        ctx.set_option("query_wg", -1)
    assert not st_d.path_flags & (LOW | QUERY_WG | FILTERED) and st_d.path_flags & GROUP, st_d.path_flags


# ---- 2. a superseded doc must not be counted -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_a_superseded_doc_is_not_counted(tiny, cols):
    """The newest column writes four docs again with only 20 of their 64 random hashes: a plain doc of column 0 (dropped among the lane's
    own words), a doc in column 2's SHARED list of 4 (a list head), one in column 3's list of 70 (read on by the wave), and a DOUBLE doc
    -- at 9 columns (lines of 4 hash values) of column 6: DOUBLE is a double in every column, 18 words, those of columns 6 .. 8 a words
    task beyond the lane's twelve.  A query of ALL the old hashes (SHARED and DOUBLE among them) at min_score 1, pct 0 gives the doc a
    score of 20: not 64 + (the old postings alone), not 84 + (both versions)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1610 + cols)
    per = 1500 if cols == 5 else 800
    dcol = 6 if cols == 9 else 1
    docs = [17, 2 * per + 3, 3 * per + 41, dcol * per + 1]
    w = World(Pair, ctx)
    # (the old versions' hashes are known only once their columns exist: two passes over the same random stream)
    rng0, older = np.random.default_rng(1610 + cols), []
    for s in range(cols - 1):
        ids = np.arange(1 + s * per, 1 + (s + 1) * per, dtype=np.int64)
        older.append(_rand_items(rng0, ids, 64, _usual(s, ids)))
    olds = {d: _rows(next(it for it in older if len(_rows(it, d))), d) for d in docs}
    kept = {d: [int(h) for h in olds[d] if int(h) not in (SHARED, DOUBLE)][:20] for d in docs}
    assert all(len(v) == 20 for v in kept.values()) and SHARED in olds[docs[1]] and SHARED in olds[docs[2]] and DOUBLE in olds[docs[3]]
    p, _ = w.columns(rng, cols, per, 64, _usual, again=kept)
    assert all(np.array_equal(_rows(next(it for it in w.items if len(_rows(it, d))), d), olds[d]) for d in docs)
    queries = [olds[d] for d in docs] + [np.concatenate([olds[d], _noise(rng, 900)]) for d in docs]
    queries += [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE]) for i in range(8)]
    got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=0))
    for i, d in enumerate(docs + docs):
        assert [s for dd, s in got[i] if dd == d] == [20], (d, [r for r in got[i] if r[0] == d], got[i][:3])
    _both(ctx, p, queries, _legacy(fpx))


# ---- 3. a tombstone at the cut ----------------------------------------------------------------------------------------------------

def test_a_tombstone_at_the_cut(tiny):
    """200 docs of column 0 (101 .. 300) share two hashes: a tie at a score of 1 for a query with one of them, of 2 with both.  A memory
    segment deletes 101 .. 105 -- the lowest ids of the tie, in the list's head -- and 150, 151 (read on by the wave).  With pct 0 and a
    limit that cuts inside the tie the quota goes to the next LIVE ids: limits 1, 7, 100 and 500, min_score 1 and 2"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1620)
    w = World(Pair, ctx)
    hashes = np.array([CROWD, CROWD + 7919], dtype=np.uint32)
    w.columns(rng, 4, 1200, 40, lambda s, ids: [(int(c), ids[100:300]) for c in hashes] if s == 0 else [])
    gone = [101, 102, 103, 104, 105, 150, 151]
    w.changes([("delete", d) for d in gone] + [("insert", 4801, rng.integers(0, 1 << 32, 30).tolist())])
    p = w.finish()
    live = [d for d in range(101, 301) if d not in gone]
    sets = [fpx.SearchOptions(max_results=k, min_score=m, min_score_pct=0) for m in (1, 2) for k in (1, 7, 100, 500)]
    queries, opts = [], []
    for i in range(16):
        q = np.concatenate([hashes[: 1 + i // 8], _noise(rng, 300)])
        rng.shuffle(q)
        queries.append(q)
        opts.append(sets[i % 8])
    got, st = _both(ctx, p, queries, opts)
    for i, (g, o) in enumerate(zip(got, opts)):
        score = 1 + i // 8
        top = [d for d, s in g if s == score and 101 <= d <= 300]
        if score < o.min_score:
            assert top == [], (i, g[:3])
        else:
            assert top == live[: o.max_results], (i, o.max_results, top[:8])
    assert [d for d, _ in got[1]] == [106, 107, 108, 109, 110, 111, 112], got[1]


# ---- 4. memory segments with the filter: ids across gmin ------------------------------------------------------------------------

@pytest.mark.parametrize("first", [100_000, (1 << 32) - 4 * 1500])
def test_memory_segments_reinsert_group_docs(tiny, first):
    """the group's columns start at doc 100 000 (or end at 0xFFFFFFFF); memory segments hold docs 5 .. 60 -- below gmin: their records
    wrap -- and write three group docs again with NEW hashes (a plain doc, one in a list of 4, one in a list of 70): the old hashes no
    longer find them, the order at the cut is the order of REAL ids"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1630 + first % 7)
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 4, 1500, 48, _usual, first=first)
    below = np.arange(5, 61)
    gone = [first + 16, first + 2 * 1500 + 2, first + 3 * 1500 + 40]
    ids0 = sorted(list(below[:30]) + gone[:2])
    w.memory(_rand_items(rng, ids0, 48, [(SHARED, below[:3])]), ids0)
    ids1 = sorted(list(below[30:]) + gone[2:])
    w.memory(_rand_items(rng, ids1, 48), ids1)
    p = w.finish()
    assert p.reader.snapshot.info()["memory"] == 2
    group_items, mem_items = np.concatenate(w.items[:4]), np.concatenate(w.items[4:6])
    one_each = np.array([int(_rows(mem_items, d)[d % 7]) for d in below], dtype=np.uint32)      # a hash of every memory doc below gmin
    queries = [np.concatenate([_rows(group_items, d), _noise(rng, 500)]) for d in gone]       # (the OLD hashes of the docs written again)
    queries += [np.concatenate([_rows(mem_items, d), _noise(rng, 500)]) for d in gone]        # (... and the new ones)
    queries += [np.concatenate([one_each, _sampled(rng, group_items, 300), _noise(rng, 100)]) for _ in range(6)]
    queries += [_aimed(rng, w.items[i % len(w.items)], 600, [SHARED, DOUBLE]) for i in range(12)]
    got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=20, min_score=1, min_score_pct=0))
    for i, d in enumerate(gone):
        assert d not in [r[0] for r in got[i]], (d, got[i][:4])
        assert got[3 + i][0] == (d, 48), (d, got[3 + i][:2])
    for g in got[6:12]:
        top = [d for d, s in g if s == 1]
        assert len(g) == 20 and top == sorted(top) and top and top[-1] <= 60, g
    _both(ctx, p, queries, _legacy(fpx))
    got, _ = _both(ctx, p, queries, fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=0))
    assert {d for d, _ in got[6]} >= set(int(d) for d in below)


# ---- 5. columns outside the snapshot ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem,dead", [(False, False), (True, False), (False, True), (True, True)])
def test_masked_columns_after_a_merge_without_regroup(tiny, mem, dead):
    """four columns in a packed group, the two oldest merged (a segment of its own next to the group, no regroup): the group keeps two
    columns outside the snapshot -- with and without superseded docs, with and without memory segments (the shapes of
    test_gpu_query_wg_filtered.py's test of the same name)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1640 + 2 * mem + dead)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 4, 2000, 48, _usual)
    merged = p.reader.snapshot.merge(p.gpu_segs[0:2], 512)
    want = p.osnap.merge(p.orc_file[0:2])
    wb, wi = oracle.build_blocks(want["items"], want["min_doc_id"], 512)
    q = World(Pair, ctx)
    q.items, q.commit = list(w.items), 10
    q.p.gpu_segs = [merged] + p.gpu_segs[2:]
    q.p.orc_file = [oracle.file_segment(wb, 512, wi, want["min_doc_id"], want["max_doc_id"], want["commit_id"], want["doc_ids"], want["doc_alive"])] + p.orc_file[2:]
    if mem:
        nxt = 8001
        for m in range(2):
            ids = list(range(nxt, nxt + 40))
            items = _rand_items(rng, ids, 30)
            if dead and m == 1:                                    # a doc of an active column written again
                items = np.unique(np.concatenate([items, _post(0, [4003]) | (_rows(w.items[2], 4003).astype(U64) << U64(32))]))
                ids.append(4003)
            q.memory(items, sorted(ids))
            nxt += 40
    elif dead:
        q.changes([("delete", 6001), ("insert", 8001, rng.integers(0, 1 << 32, 30).tolist())])
    q.finish()
    info = q.p.reader.snapshot.info()
    assert info["groups"] == 1, info
    allitems = np.concatenate(w.items)
    queries = [np.concatenate([_rows(allitems, d), _noise(rng, 900)]) for d in (17, 2500, 4003, 6001)]     # (docs of the merged columns, of both active ones)
    queries += [_aimed(rng, q.items[i % len(q.items)], 1000, [SHARED, DOUBLE]) for i in range(20)]
    for opts in (_legacy(fpx), fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0)):
        got, st = _both(ctx, q.p, queries, opts, want=TAKEN | TWO_PARTS)
    assert got[0][0][0] == 17 and got[1][0][0] == 2500 and [d for d, _ in got[0]].count(17) == 1      # (found in the merged segment, once)
    assert (6001 not in [d for d, _ in got[3]]) if (dead and not mem) else got[3][0][0] == 6001


# ---- 6. two parts -----------------------------------------------------------------------------------------------------------------

def test_two_parts(tiny):
    """a filtered part 0 -- a group of 5 columns whose dead sets hold the docs of part 1 -- next to two checkpoints in blocks, one of which
    tombstones a group doc and one of which re-inserts one, and a segment direct-addressed alone: bits 12, 8, 7 and 6; the same batch
    resident in HBM"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1650)
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 5, 1500, 64, _usual)
    bounds = [(1, nxt)]
    for s in range(2):
        ids, alive = list(range(nxt, nxt + 800)), [1] * 800
        items = _rand_items(rng, ids, 64, [(SHARED, ids[:7])])
        if s == 0:
            ids.insert(0, 5); alive.insert(0, 0)                   # doc 5 of the group: a tombstone
        else:                                                      # ... and doc 1509 written again, with its own hashes
            items = np.unique(np.concatenate([items, _post(0, [1509]) | (_rows(w.items[1], 1509).astype(U64) << U64(32))]))
            ids.insert(0, 1509); alive.insert(0, 1)
        w.file(items, ids, form="blocks", alive=np.array(alive, dtype=np.uint8))
        nxt += 800
    bounds.append((bounds[-1][1], nxt))
    ids = np.arange(nxt, nxt + 2000)
    w.file(_rand_items(rng, ids, 64, [(SHARED, ids[:70])]), ids, form="alone")
    nxt += 2000
    bounds.append((bounds[-1][1], nxt))
    p = w.finish()
    assert not any(g.grouped for g in p.gpu_segs[5:8]) and bool(p.gpu_segs[7].direct) and not p.gpu_segs[5].direct, [g.layout_reason for g in p.gpu_segs]
    queries = [np.concatenate([_rows(w.items[0], 5), _noise(rng, 900)]), np.concatenate([_rows(w.items[1], 1509), _noise(rng, 900)])]
    queries += [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(38)]
    got, st = _both(ctx, p, queries, _legacy(fpx), want=TAKEN | TWO_PARTS)
    assert 5 not in [d for d, _ in got[0]] and got[1][0][0] == 1509 and [d for d, _ in got[1]].count(1509) == 1, (got[0][:2], got[1][:2])
    found_in = [sum(1 for g in got if g and lo <= g[0][0] < hi) for lo, hi in bounds]
    assert all(n >= 3 for n in found_in), found_in
    _both(ctx, p, queries, fpx.SearchOptions(max_results=7, min_score=1, min_score_pct=0), want=TAKEN | TWO_PARTS)
    # resident in HBM: the same path, the same answers
    ctx.set_option("query_wg", 2)
    ctx.set_option("low_wg", 2)
    try:
        want, _ = p.reader.search_batch(queries, _legacy(fpx))
        qb = fpx.QueryBatch(ctx, queries=queries, options=_legacy(fpx))
        o, n, st_r = fpx.search_resident(p.reader, qb)
        qb.release()
        assert st_r.path_flags & (TAKEN | TWO_PARTS) == TAKEN | TWO_PARTS, st_r.path_flags
        assert fpx.results_to_lists(o, n) == want
    finally:
        ctx.set_option("low_wg", -1)
        ctx.set_option("query_wg", -1)


# ---- 7. mixed floors in one batch -----------------------------------------------------------------------------------------------

@pytest.fixture
def shapes(tiny):
    """five columns, the hashes 0 and 0xFFFFFFFF in three of them; the newest writes docs 300 and 17 of column 0 again"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1660)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 5, 1500, 64, lambda s, ids: _usual(s, ids) + [(0, ids[:2]), (0xFFFFFFFF, ids[5:8])][: 2 if s % 2 == 0 else 0],
                     again={300: None, 17: None})
    return fpx, ctx, rng, w, p


def test_mixed_floors_in_one_batch(shapes):
    """explicit floors 1, 2, 3 and 50 and the default one; lengths 0, 1, 2, 40, 41 (default floors 2 and 3), 256, 257 and 4096;
    duplicates inside a query; the hashes 0 and 0xFFFFFFFF.  A batch with no low query: the filtered k_search_query, bit 8 without bit 12"""
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
    for m in (2, None):
        _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=m, min_score_pct=0))
    got, _ = _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0))
    assert got[0] == [] and got[1][0] == (300, 1) and got[5][0] == (300, len(own)) and got[9][0] == (300, len(own))
    # a batch in which NO query is low: the filtered k_search_query, whatever the option says
    high = [q for q in shapes_ if len(q) > 40]
    _both(ctx, p, high, fpx.http_options(), want=QUERY_WG | GROUP | FILTERED, want_not=LOW)
    _both(ctx, p, shapes_, fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0), want=QUERY_WG | GROUP | FILTERED, want_not=LOW)


# ---- 8. more queries than workgroups --------------------------------------------------------------------------------------------

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


# ---- 9. record counts at the array's edges, hand-backs --------------------------------------------------------------------------

@pytest.fixture
def edges(tiny):
    """8 columns; HOT8 has 1000 docs in each of them, HOT1 1000 docs in column 0; column 1 holds 3500 hashes of one doc each, column 3
    600 hashes with a list of three docs each; the newest column writes doc 1 of column 0 -- a HOT8 doc -- again"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1670)
    w = World(Pair, ctx)
    singles = [SINGLE + 7919 * k for k in range(3500)]
    lists = [LISTS + 7919 * k for k in range(600)]

    def extra(s, ids):
        e = [(HOT8, ids[:1000])]
        if s == 0:
            e.append((HOT1, ids[200:1200]))
        if s == 1:
            e += [(h, ids[i % len(ids): i % len(ids) + 1]) for i, h in enumerate(singles)]
        if s == 3:
            e += [(h, ids[1100:1103]) for h in lists]
        return e

    p, _ = w.columns(rng, 8, 1200, 24, extra, again={1: None})
    return fpx, ctx, rng, w, p, np.array(singles, dtype=np.uint32), np.array(lists, dtype=np.uint32)


def _records(p, q):
    """the query's LIVE hit records -- what the kernel's array holds: the scores of everything a floor of 1 returns"""
    return sum(s for _, s in p.osnap.search(q, 1 << 20, 1, 0))


_exact = functools.partial(wg.exact, _records)


def test_record_counts_at_the_arrays_edges(edges):
    """255, 256, 257 and 4097 live records (the network's smallest size, and the power of two above 4096), 8150 (just under the array's
    8192: HOT8's 8001 postings, one of them superseded), and a size for each network in between"""
    fpx, ctx, rng, w, p, singles, lists = edges
    sizes = (([], 255), ([], 256), ([], 257), ([HOT1], 4097), ([HOT8], 8150), ([], 600), ([], 1500), ([], 3000))
    queries = [_exact(p, rng, head, singles, target) for head, target in sizes]
    assert [_records(p, q) for q in queries] == [t for _, t in sizes]
    assert p.osnap.search(queries[4], 40, 1, 0, with_stats=True)[1].scanned_docs == 8151       # (counted before supersession)
    for i in range(7):
        q = _aimed(rng, w.items[i % 8], 300)
        queries.append(q[(q != HOT8) & (q != HOT1)])
    for opts in (fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0), fpx.SearchOptions(max_results=500, min_score=2, min_score_pct=0), _legacy(fpx)):
        got, st = _both(ctx, p, queries, opts)


def _hands_back(fpx, ctx, p, plain, heavy, opts):
    """`plain` is taken; `heavy` -- the same batch with one query too large -- is the pipeline's, and so is the next batch of that snapshot
    (the back-off); a fresh snapshot takes the kernel again"""
    got, st = _both(ctx, p, plain, opts)
    ctx.set_option("query_wg", 2)
    ctx.set_option("low_wg", 2)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & (LOW | QUERY_WG | FILTERED) and st_h.path_flags & GROUP, f"not handed back ({st_h.path_flags})"
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, opts.max_results, opts.min_score, opts.min_score_pct)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernel)
        assert not st_n.path_flags & (LOW | QUERY_WG) and got_n == got, st_n.path_flags
        ctx.set_option("low_wg", 0)
        got_p, st_p = p.reader.search_batch(heavy, opts)
        assert got_p == got_h and _figures(st_p) == _figures(st_h)
    finally:
        ctx.set_option("low_wg", -1)
        ctx.set_option("query_wg", -1)
    ctx.set_option("query_wg", 2)
    try:
        p.finish()                                             # a fresh snapshot of the same segments
    finally:
        ctx.set_option("query_wg", -1)
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


def _plain(rng, w, n):
    qs = [_aimed(rng, w.items[i % 8], 300) for i in range(n)]
    return [q[(q != HOT8) & (q != HOT1)] for q in qs]


def test_records_beyond_the_array_are_handed_back(edges):
    """HOT8 and a few hundred more: 8300 live records, over the array's 8192"""
    fpx, ctx, rng, w, p, singles, lists = edges
    plain = _plain(rng, w, 12)
    heavy = list(plain)
    heavy[5] = np.concatenate([[HOT8], singles[:300]]).astype(np.uint32)
    assert _records(p, heavy[5]) == 8300
    _hands_back(fpx, ctx, p, plain, heavy, fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0))


def test_tasks_beyond_the_filtered_queue_are_handed_back(edges):
    """a query of 512 hashes with a list each fills the filtered form's task queue (QS_TASKS_FILT: each task has a word of its words' columns
    behind the queue) and is taken; one of 513 overflows it -- 1539 records, far from the array's end -- and hands the batch back"""
    fpx, ctx, rng, w, p, singles, lists = edges
    plain = _plain(rng, w, 12)
    plain[3] = lists[:QS_TASKS_FILT].copy()
    heavy = list(plain)
    heavy[5] = lists[: QS_TASKS_FILT + 1].copy()
    assert _records(p, plain[3]) == 3 * QS_TASKS_FILT and _records(p, heavy[5]) == 3 * QS_TASKS_FILT + 3
    _hands_back(fpx, ctx, p, plain, heavy, fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0))


# ---- 10. gating -----------------------------------------------------------------------------------------------------------------

def test_gating(shapes, tiny):
    """low_wg = 2 with query_wg = 1 on the filtered group: the pipeline, as under low_wg = 0.  low_wg = 2 on a CLEAN group is low_wg = 1:
    k_search_low, bit 12 without bit 8 -- under query_wg 1 and 2.  (low_wg = 1 with query_wg = 2 on the filtered group:
    test_gpu_low_wg.py::test_a_filtered_group_with_low_floors_is_the_pipelines)"""
    fpx, ctx, rng, w, p = shapes
    queries = [_aimed(rng, w.items[i % 5], 600, [SHARED]) for i in range(8)]
    _both(ctx, p, queries, _legacy(fpx), want=GROUP, want_not=LOW | FILTERED | QUERY_WG, query_wg=1)
    _both(ctx, p, queries, _legacy(fpx))                      # (query_wg 2: taken)
    clean = World(tiny[2], ctx)
    pc, _ = clean.columns(rng, 5, 1500, 64, _usual)
    queries = [_aimed(rng, clean.items[i % 5], 600, [SHARED]) for i in range(8)]
    for query_wg in (1, 2):
        _both(ctx, pc, queries, _legacy(fpx), want=LOW | QUERY_WG | GROUP, want_not=FILTERED, query_wg=query_wg)
