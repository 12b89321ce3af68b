"""k_search_low_coop (csrc/fpx_qsearch.hpp, option low_wg = 3 with filt_coop = 1 under query_wg = 2): a batch with queries whose score floor
is 1 or 2 -- the legacy protocol's min_score 1, the default floor of a query of 40 hashes or fewer -- on ONE packed group that is FILTERED
(superseded docs and/or columns outside the snapshot), searched by k_search_filt's rounds and tasks -- eight lanes to a line behind the
group's union dead-set bitmap -- with k_search_low's sorted tail behind them.  fpx_stats.path_flags: bit 12 (4096) the sorted tail and bit
16 (65536) eight lanes behind the union bitmap TOGETHER, with bit 8 (256) the filtered form, bit 6 (64) a query per workgroup and bit 2
(4) a group; bit 7 (128) where it was part 0 of a snapshot in two parts.  Whatever does not meet the condition -- a snapshot made under
filt_coop = 0, an id range no bitmap spans, several groups, a clean group -- behaves under low_wg = 3 exactly as under 2.

Every case goes through wg_harness.both(..., "low_wg", 3, ...) with query_wg = 2 and filt_coop = 1: Pair.check (results and every query's
scanned blocks / docs == the oracle's) with the path bits asserted, then the batch under low_wg 3 and under 0 -- the pipeline -- compared.
The same batch then runs under low_wg = 2 (k_search_low_filt: the same path bits but bit 16) and under query_wg = 0 (the pipeline, one
part), compared byte for byte: results, scanned_blocks, scanned_docs, probes, hits, algorithmic_bytes, per-query blocks / docs and the
growth of the context's scan histograms, nothing unbucketed (probes, hits and the histograms not against query_wg = 0 where the snapshot
was in two parts: the parts count a probe each).  Snapshots are made with FPX_FILT_COOP=1 in the environment (the option's fallback).
The groups are tiny (group_packed = 1, FPX_DIRECT_MIN_ITEMS = 0): 5 columns give lines of 8 hash values, 9 columns lines of 4; each case
is the smallest shape that reaches its branch.  Worlds 1 and 3 and the wide id range are tests/test_gpu_filt_coop.py's, a second group is
made the way tests/test_gpu_groups_wg.py makes one.

FAILS ON THE PARENT: test_legacy_options_on_every_kind_of_word_superseded.  There set_option("low_wg", 3) is accepted (only a minimum is
checked) but the value is compared == 2 and == 1, so the batch is the pipeline's and the path-bit assertion fails.

MUTANTS (each built once by hand and run against cases 1 - 9 of this file, 21 tests; none committed):
  * round_coop never tests the union bitmap (`if (ub != nullptr)` made false: a superseded inline word is kept) -- 18 of the 21 fail:
    every_kind_of_word_superseded[5, 9], a_superseded_doc_is_not_counted[5, 9], a_whole_line_superseded, masked_columns[5-True],
    a_mixed_batch[5, 9], memory_segments_rewrite_and_delete (all four), wide_ids (all four), query_shapes[5, 9].  The three that pass
    have no superseded INLINE word: masked_columns[5-False, 9-False] (no dead set) and superseded_docs_at_the_cut (its dead docs are
    in a list: the tasks phase's test, not the mutant's).
  * the hash's lane does not cut the words of columns outside the snapshot out of the line's mask (`wr &= am << wb` dropped) -- the three
    masked_columns cases fail, the other 18 pass."""
import numpy as np
import pytest

import wg_harness as wg
from test_gpu_filt_coop import COOP, LINE4, _extra, _old, _world1, _world1_queries, _world3
from test_gpu_groups_wg import _finish, _layout, _more
from wg_harness import (FILTERED, GROUP, LOW, QS_MAX_HASHES, QS_TASKS_FILT, QUERY_WG, TWO_PARTS, U64, HOT8, HOT1,
                        aimed as _aimed, figures as _figures, legacy as _legacy, noise as _noise, post as _post, rand_items as _rand_items,
                        rows as _rows, sampled as _sampled)

pytestmark = pytest.mark.gpu

SHARED, DOUBLE, CROWD, SINGLE, LISTS = 0x2BADF00D, 0x37770000, 0x51515151, 0x70000000, 0x19000000
GROUPS = 8192                       # fpx_stats.path_flags bit 13
TAKEN = LOW | COOP | FILTERED | QUERY_WG | GROUP
LOW_FILT = LOW | FILTERED | QUERY_WG | GROUP                 # k_search_low_filt: what low_wg = 2 runs
OPTIONS = ("low_wg", "filt_coop", "groups_wg", "hot_wg", "query_wg", "direct_min_items")
_usual = wg.usual(SHARED, DOUBLE)


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.fixture
def tiny(env, monkeypatch):
    """every file segment a direct-addressed candidate unless a test says otherwise, groups packed; filt_coop = 1 through its fallback"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1) as e:
        monkeypatch.setenv("FPX_FILT_COOP", "1")
        yield e


def World(Pair, ctx, **kw):
    return wg.World(Pair, ctx, packed=1, snapshot_query_wg=2, **kw)


def _both(ctx, p, queries, opts, want=TAKEN, want_not=0, query_wg=2, also=(), parts=False):
    """wg.both under low_wg = 3 (query_wg, filt_coop = 1 and `also` around it) against low_wg = 0; then the batch under low_wg 3, under 2 and
    under query_wg = 0, everything equal.  Under 2 the path bits are those under 3 without bit 16"""
    also = [("query_wg", query_wg), ("filt_coop", 1)] + list(also)
    low_taken = bool(want & LOW)
    got, st = wg.both(ctx, p, queries, opts, "low_wg", 3, clear=LOW | ((QUERY_WG | COOP) if low_taken else 0), want=want, want_not=want_not,
                      also=also, compare=wg.WITH_BYTES)
    try:
        for name, value in also:
            ctx.set_option(name, value)
        ctx.set_option("low_wg", 3)
        h0, _ = wg.hist(ctx)
        g3, s3, qb3, qd3 = p.reader.search_batch_stats(queries, opts)
        h1, unb1 = wg.hist(ctx)
        ctx.set_option("low_wg", 2)
        g2, s2, qb2, qd2 = p.reader.search_batch_stats(queries, opts)
        h2, unb2 = wg.hist(ctx)
        ctx.set_option("low_wg", -1)
        ctx.set_option("query_wg", 0)
        g0, s0, qb0, qd0 = p.reader.search_batch_stats(queries, opts)
        h3, unb3 = wg.hist(ctx)
    finally:
        ctx.set_option("low_wg", -1)
        for name, _ in also:
            ctx.set_option(name, -1)
    print(f"low_wg 3: path_flags {s3.path_flags}, {_figures(s3)}; low_wg 2: {s2.path_flags}, {_figures(s2)}; query_wg 0: {s0.path_flags}, {_figures(s0)}")
    assert s3.path_flags & want == want and not s3.path_flags & want_not, (s3.path_flags, want, want_not)
    assert s2.path_flags == s3.path_flags & ~(COOP if low_taken else 0), (s2.path_flags, s3.path_flags)
    assert not s0.path_flags & (QUERY_WG | TWO_PARTS | FILTERED | COOP | LOW), s0.path_flags
    assert g3 == got and g2 == got and g0 == got
    assert _figures(s3) == _figures(st) and _figures(s2) == _figures(s3), (_figures(st), _figures(s3), _figures(s2))
    assert [int(x) for x in qb2] == [int(x) for x in qb3] and [int(x) for x in qd2] == [int(x) for x in qd3]
    assert wg.growth(h0, h1) == wg.growth(h1, h2), (wg.growth(h0, h1), wg.growth(h1, h2))
    assert [int(x) for x in qb0] == [int(x) for x in qb3] and [int(x) for x in qd0] == [int(x) for x in qd3]
    assert (s0.scanned_blocks, s0.scanned_docs, s0.algorithmic_bytes) == (s3.scanned_blocks, s3.scanned_docs, s3.algorithmic_bytes)
    if not parts:
        assert _figures(s0) == _figures(s3), (_figures(s0), _figures(s3))
        assert wg.growth(h2, h3) == wg.growth(h0, h1), (wg.growth(h2, h3), wg.growth(h0, h1))
    assert unb1 == 0 and unb2 == 0 and unb3 == 0, (unb1, unb2, unb3)
    return got, st


def _low1(fpx, k=500):
    return fpx.SearchOptions(max_results=k, min_score=1, min_score_pct=0)


# ---- 1. the legacy options where every kind of word is superseded ----------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_legacy_options_on_every_kind_of_word_superseded(tiny, cols):
    """test_gpu_filt_coop's world 1 under the legacy options: the newest column writes again a plain inline word's doc, both words of
    doubles, a list's head, a doc of a list read on by the wave and, at nine columns, a doc whose words are in `ext`.  Bits 12 | 16 | 8 | 6
    | 2; each rewritten doc comes back exactly once.  The test that FAILS ON THE PARENT: there low_wg = 3 is accepted but compared == 2,
    the batch is the pipeline's and the path-bit assertion fails (confirmed once with the parent commit's library: path_flags 4 at five
    columns, 7 at nine -- the group, by the pipeline --, AssertionError (4, 69956, 0) and (7, 69956, 0))"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2500 + cols)
    w, p, again = _world1(Pair, ctx, rng, cols)
    assert p.reader.snapshot.info()["dead_union_bytes"] == 4 * (((cols * 1500 - 1) >> 5) + 1), p.reader.snapshot.info()
    queries = _world1_queries(rng, w, again, cols, 28)
    for opts in (_legacy(fpx), _low1(fpx)):
        got, st = _both(ctx, p, queries, opts)
        for i, d in enumerate(again):
            assert got[i] and got[i][0][0] == d and [r[0] for r in got[i]].count(d) == 1, (d, got[i][:4])
    # off by default: such a batch is the pipeline's, under query_wg 2 and filt_coop 1 as well
    ctx.set_option("query_wg", 2)
    ctx.set_option("filt_coop", 1)
    try:
        assert ctx.get_option("low_wg") == 0
        _, st_d = p.reader.search_batch(queries, _legacy(fpx))
    finally:
        ctx.set_option("filt_coop", -1)
        ctx.set_option("query_wg", -1)
    assert not st_d.path_flags & (LOW | QUERY_WG | FILTERED | COOP) and st_d.path_flags & GROUP, st_d.path_flags


# ---- 2. a superseded doc must not be counted -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_a_superseded_doc_is_not_counted(tiny, cols):
    """test_gpu_low_wg_filtered's world of the same name: the newest column writes four docs again with only 20 of their 64 hashes -- a plain
    doc, one in a list of 4 (a list's head), one in a list of 70 (read on by the wave), a DOUBLE doc (at nine columns in `ext`).  A query
    of ALL the old hashes at min_score 1, pct 0 gives the doc a score of 20: not 64 (the old postings), not 84 (both versions)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2510 + cols)
    per = 1500 if cols == 5 else 800
    dcol = 6 if cols == 9 else 1
    docs = [17, 2 * per + 3, 3 * per + 41, dcol * per + 1]
    w = World(Pair, ctx)
    rng0, older = np.random.default_rng(2510 + cols), []         # (the old versions' hashes: two passes over the same random stream)
    for s in range(cols - 1):
        ids = np.arange(1 + s * per, 1 + (s + 1) * per, dtype=np.int64)
        older.append(_rand_items(rng0, ids, 64, _usual(s, ids)))
    olds = {d: _rows(next(it for it in older if len(_rows(it, d))), d) for d in docs}
    kept = {d: [int(h) for h in olds[d] if int(h) not in (SHARED, DOUBLE)][:20] for d in docs}
    assert all(len(v) == 20 for v in kept.values()) and SHARED in olds[docs[1]] and SHARED in olds[docs[2]] and DOUBLE in olds[docs[3]]
    p, _ = w.columns(rng, cols, per, 64, _usual, again=kept)
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0
    queries = [olds[d] for d in docs] + [np.concatenate([olds[d], _noise(rng, 900)]) for d in docs]
    queries += [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE]) for i in range(16)]
    got, st = _both(ctx, p, queries, _low1(fpx))
    for i, d in enumerate(docs + docs):
        assert [s for dd, s in got[i] if dd == d] == [20], (d, [r for r in got[i] if r[0] == d], got[i][:3])
    _both(ctx, p, queries, _legacy(fpx))


# ---- 3. a whole line superseded --------------------------------------------------------------------------------------------------------

def test_a_whole_line_superseded(tiny):
    """test_gpu_filt_coop's world: nine columns, the four hash values of ONE line each have a doc in the seven oldest columns -- 28 inline
    words --, and the newest column writes all seven docs again with other hashes: all eight lanes of a group hold dead words of that
    line.  At a floor of 1 a single old posting counted would return its doc"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2520)
    per = 1500
    w = World(Pair, ctx)
    gone = [s * per + 11 for s in range(7)]
    fresh = {d: rng.integers(0, 1 << 32, 48, dtype=U64).tolist() for d in gone}
    p, _ = w.columns(rng, 9, per, 48, lambda s, ids: _usual(s, ids) + ([(LINE4 + k, ids[10:11]) for k in range(4)] if s < 7 else []), again=fresh)
    line = np.arange(LINE4, LINE4 + 4, dtype=np.uint32)
    queries = [np.concatenate([line, _noise(rng, 900)]), np.concatenate([line, line, _rows(w.items[0], 11), _noise(rng, 500)])]
    queries += [np.concatenate([np.asarray(fresh[d], dtype=np.uint32), line, _noise(rng, 600)]) for d in gone]
    queries += [_aimed(rng, w.items[i % 9], 1000, [SHARED, DOUBLE, LINE4 + i % 4]) for i in range(16)]
    got, st = _both(ctx, p, queries, _low1(fpx))
    assert not any(r[0] in gone for r in got[0] + got[1]), (got[0][:4], got[1][:4])
    for i, d in enumerate(gone):
        assert got[2 + i][0] == (d, 48) and [r[0] for r in got[2 + i]].count(d) == 1, (d, got[2 + i][:3])
    _both(ctx, p, queries, _legacy(fpx))


# ---- 4. masked columns -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,dead", [(5, False), (9, False), (5, True)])
def test_masked_columns_after_a_merge_without_regroup(tiny, cols, dead):
    """the two oldest columns merged away (a segment of its own next to the group, no regroup): their words share lines with the active
    columns' and give nothing -- the hash's lane cuts them out of the line's mask.  Without a dead set anywhere there is no bitmap
    (dead_union_bytes == 0, a null pointer) and the kernel is k_search_low_coop all the same; with one both masks work together"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2530 + cols + dead)
    per = 1500
    w = World(Pair, ctx)
    p, nxt = w.columns(rng, cols, per, 48, _usual)
    merged = p.reader.snapshot.merge(p.gpu_segs[0:2], 512)
    want = p.osnap.merge(p.orc_file[0:2])
    wb, wi = oracle.build_blocks(want["items"], want["min_doc_id"], 512)
    q = World(Pair, ctx)
    q.items, q.commit = list(w.items), 20
    q.p.gpu_segs = [merged] + p.gpu_segs[2:]
    q.p.orc_file = [oracle.file_segment(wb, 512, wi, want["min_doc_id"], want["max_doc_id"], want["commit_id"], want["doc_ids"], want["doc_alive"])] + p.orc_file[2:]
    if dead:
        q.changes([("delete", 2 * per + 1), ("delete", 3 * per + 41), ("insert", nxt, rng.integers(0, 1 << 32, 30).tolist())])
    q.finish()
    info = q.p.reader.snapshot.info()
    assert info["groups"] == 1 and (info["dead_union_bytes"] != 0) == dead, info
    queries = [_old(w, d, rng) for d in (17, per + 500, 2 * per + 1, 3 * per + 41, 2 * per + 2)]
    queries += [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE]) for i in range(20)]
    for opts in (_legacy(fpx), _low1(fpx, 80)):
        got, st = _both(ctx, q.p, queries, opts, want=TAKEN | TWO_PARTS, parts=True)
    assert got[0][0][0] == 17 and got[1][0][0] == per + 500 and [r[0] for r in got[0]].count(17) == 1     # (found in the merged segment, once)
    assert got[4][0][0] == 2 * per + 2
    for i, d in ((2, 2 * per + 1), (3, 3 * per + 41)):
        assert (d not in [r[0] for r in got[i]]) if dead else got[i][0][0] == d, (d, got[i][:3])


# ---- 5. both tails in one launch -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_a_mixed_batch(tiny, cols):
    """world 1: ONE legacy query among queries with floors above 2, and one with a floor of 3 among legacy ones -- the sorted tail and the
    usual one (filter, sweep, exact table) take turns in a workgroup's queries.  A batch without a low floor is k_search_filt's, whatever
    low_wg says: bit 16 without bit 12"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2540 + cols)
    w, p, again = _world1(Pair, ctx, rng, cols)
    queries = _world1_queries(rng, w, again, cols, 24)
    high = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    for one, rest in ((_legacy(fpx), high), (high, _legacy(fpx)), (_low1(fpx, 7), fpx.http_options())):
        for at in (0, 13):
            opts = [one if i == at else rest for i in range(len(queries))]
            got, st = _both(ctx, p, queries, opts)
            for i, d in enumerate(again):
                assert got[i] and got[i][0][0] == d and [r[0] for r in got[i]].count(d) == 1, (d, got[i][:4])
    _both(ctx, p, queries, high, want=COOP | FILTERED | QUERY_WG | GROUP, want_not=LOW)


# ---- 6. memory segments, and two parts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
@pytest.mark.parametrize("parts", [False, True], ids=["one_part", "two_parts"])
def test_memory_segments_rewrite_and_delete(tiny, cols, parts):
    """memory segments write docs of three columns again with new hashes (a plain doc, one in a list of 4, one in a list of 70) and
    delete one doc of EVERY column: the MEM instantiations, every column with a dead set.  two_parts: the same with a checkpoint in
    blocks next to the group, which tombstones one more group doc -- part 0 is the filtered group: bit 7"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2550 + cols + 16 * parts)
    per = 1500
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, cols, per, 48, _usual)
    tomb = 4 * per + 77
    if parts:
        ids, alive = list(range(nxt, nxt + 600)), [1] * 600
        items = _rand_items(rng, ids, 40, [(SHARED, ids[:7])])
        ids.insert(0, tomb); alive.insert(0, 0)
        w.file(items, ids, form="blocks", alive=np.array(alive, dtype=np.uint8))
        nxt += 600
    again = [17, 2 * per + 3, 3 * per + 41]
    deleted = [s * per + 9 for s in range(cols)]
    for m in range(3):
        ids = list(range(nxt, nxt + 50)) + (again if m == 1 else [])
        w.memory(_rand_items(rng, ids, 40), sorted(ids))
        nxt += 50
    w.changes([("delete", d) for d in deleted] + [("insert", nxt, rng.integers(0, 1 << 32, 30).tolist())])
    p = w.finish()
    info = p.reader.snapshot.info()
    assert info["memory"] == 4 and info["dead_union_bytes"] != 0, info
    mem_items = np.concatenate(w.items[-3:])
    queries = [_old(w, d, rng) for d in again + deleted[:3] + [tomb]]
    queries += [np.concatenate([_rows(mem_items, d), _noise(rng, 300)]) for d in again]             # (the new hashes)
    queries += [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(16)]
    for opts in (_legacy(fpx), _low1(fpx, 100)):
        got, st = _both(ctx, p, queries, opts, want=TAKEN | (TWO_PARTS if parts else 0), want_not=0 if parts else TWO_PARTS, parts=parts)
        for i, d in enumerate(again + deleted[:3]):
            assert d not in [r[0] for r in got[i]], (d, got[i][:3])
        assert (tomb not in [r[0] for r in got[6]]) if parts else got[6][0][0] == tomb, got[6][:3]
        for i, d in enumerate(again):
            assert got[7 + i][0] == (d, 40), (d, got[7 + i][:2])
        assert not any(r[0] in deleted for g in got for r in g), "a deleted doc was returned"


# ---- 7. the cut at max_results ---------------------------------------------------------------------------------------------------------

def test_superseded_docs_at_the_cut(tiny):
    """200 docs of column 0 (101 .. 300) share two hashes: a tie at a score of 1 for a query with one of them, of 2 with both.  A memory
    segment deletes 101 .. 105 -- the lowest ids of the tie, in the list's head -- and 150, 151 (read on by the wave).  With pct 0 and a
    limit that cuts inside the tie the quota goes to the next LIVE ids, in id order: limits 1, 7, 100 and 500, min_score 1 and 2"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2560)
    w = World(Pair, ctx)
    hashes = np.array([CROWD, CROWD + 7919], dtype=np.uint32)
    w.columns(rng, 4, 1200, 40, lambda s, ids: [(int(c), ids[100:300]) for c in hashes] if s == 0 else [])
    gone = [101, 102, 103, 104, 105, 150, 151]
    w.changes([("delete", d) for d in gone] + [("insert", 4801, rng.integers(0, 1 << 32, 30).tolist())])
    p = w.finish()
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0
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


# ---- 8. wide ids -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
@pytest.mark.parametrize("high", [False, True], ids=["from_1", "to_0xFFFFFFFF"])
def test_wide_ids(tiny, cols, high):
    """test_gpu_filt_coop's bitmap edges -- a memory segment writes again, with new hashes, the group's docs gmin, gmin + 31, gmin + 32 and
    its largest id -- with ids from 1 and ids up to 0xFFFFFFFF (a gmin near 2^32: neither gmin + word nor the bitmap's index may wrap).
    to_0xFFFFFFFF: the memory segment also holds docs 5 .. 34, BELOW gmin -- their records wrap, the sorted tail orders real ids: with
    min_score 1, pct 0 and a limit of 20 the tie at a score of 1 goes to the memory docs, in id order"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2570 + cols + high)
    per = 1500
    first = ((1 << 32) - cols * per) if high else 1
    w = World(Pair, ctx)
    w.columns(rng, cols, per, 48, _usual, first=first)
    last = first + cols * per - 1
    assert not high or (first >= 0xFFFF0000 and last == 0xFFFFFFFF)
    gone = [first, first + 31, first + 32, last]
    below = list(range(5, 35)) if high else []
    ids = sorted(below + gone)
    w.memory(_rand_items(rng, ids, 48, [(SHARED, below[:3])] if high else []), ids)
    p = w.finish()
    info = p.reader.snapshot.info()
    assert info["memory"] == 1 and info["dead_union_bytes"] == 4 * (((last - first) >> 5) + 1), info
    near = [first + 1, first + 30, first + 33, last - 1]
    group_items, mem_items = np.concatenate(w.items[:cols]), w.items[-1]
    queries = [_old(w, d, rng) for d in gone] + [_old(w, d, rng) for d in near]
    queries += [np.concatenate([_rows(mem_items, d), _noise(rng, 500)]) for d in gone]              # (the new hashes)
    queries += [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE]) for i in range(10)]
    if high:
        one_each = np.array([int(_rows(mem_items, d)[d % 7]) for d in below], dtype=np.uint32)      # a hash of every memory doc below gmin
        queries += [np.concatenate([one_each, _sampled(rng, group_items, 300), _noise(rng, 100)]) for _ in range(4)]
    for opts in (_legacy(fpx), _low1(fpx, 20)):
        got, st = _both(ctx, p, queries, opts)
        for i, d in enumerate(gone):
            assert d not in [r[0] for r in got[i]], (d, got[i][:3])
            assert got[8 + i][0] == (d, 48), (d, got[8 + i][:2])
        for i, d in enumerate(near):
            assert got[4 + i] and got[4 + i][0][0] == d, (d, got[4 + i][:2])
    if high:
        for g in got[22:26]:
            top = [d for d, s in g if s == 1]
            assert len(g) == 20 and top == sorted(top) and top and top[-1] < 35, g


# ---- 9. query shapes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_query_shapes(tiny, cols):
    """1, 40, 41, 255, 256, 257, 1025 and 4096 hashes, duplicates inside a query: lanes without a probe in a round, the rolling window
    beyond 1024 hashes.  Under an explicit floor of 1 every query takes the sorted tail; under the defaults those of 1 and 40 hashes do
    (a floor of 2) and the one of 41 does not (3)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2580 + cols)
    w, p, again = _world1(Pair, ctx, rng, cols)
    own = _rows(w.items[0], 17)
    special = np.array([SHARED, DOUBLE, DOUBLE + 1, SHARED], dtype=np.uint32)
    shapes = [own[:1], np.concatenate([own[:30], _noise(rng, 10)]), np.concatenate([own[:30], _noise(rng, 11)])]
    for n in (255, 256, 257, 1025, QS_MAX_HASHES):
        q = np.concatenate([own, own[:9], special, _noise(rng, n - len(own) - 9 - len(special))])
        rng.shuffle(q)
        shapes.append(q)
    shapes += [np.full(500, int(own[0]), dtype=np.uint32), np.concatenate([_old(w, 3 * 1500 + 41, rng, 2000), special])]
    assert [len(x) for x in shapes[:8]] == [1, 40, 41, 255, 256, 257, 1025, 4096]
    for opts in (_low1(fpx, 100), fpx.http_options(), _legacy(fpx)):
        got, st = _both(ctx, p, shapes, opts)
        if opts.min_score != 1:                                # (the default floors: up to the oracle, which _both asked)
            continue
        assert got[0][0] == (17, 1) and got[1][0] == (17, 30) and got[2][0] == (17, 30), [g[:1] for g in got[:3]]
        assert all(g[0] == (17, len(own)) for g in got[3:8]), [g[:1] for g in got[3:8]]      # (a duplicate is no probe)
        assert got[8][0] == (17, 1) and [r[0] for r in got[8]].count(17) == 1, got[8][:3]


# ---- 10. fallbacks keep their kernels under low_wg = 3 ---------------------------------------------------------------------------------

def test_a_snapshot_made_under_filt_coop_0_keeps_k_search_low_filt(tiny, monkeypatch):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2590)
    monkeypatch.setenv("FPX_FILT_COOP", "0")
    w, p, again = _world1(Pair, ctx, rng, 5)
    assert p.reader.snapshot.info()["dead_union_bytes"] == 0
    queries = _world1_queries(rng, w, again, 5, 24)
    _both(ctx, p, queries, _legacy(fpx), want=LOW_FILT, want_not=COOP)
    monkeypatch.setenv("FPX_FILT_COOP", "1")
    w.finish()                                                 # (a fresh snapshot under 1: taken)
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0
    _both(ctx, p, queries, _legacy(fpx))


def test_an_id_range_beyond_2_to_the_29_keeps_k_search_low_filt(tiny):
    """two columns, ids from 1 and from 2^30; the second writes doc 17 of the first again: no bitmap over a range that wide"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2591)
    w = World(Pair, ctx)
    ids0 = np.arange(1, 1501, dtype=np.int64)
    w.file(_rand_items(rng, ids0, 48, _usual(0, ids0)), ids0, form="column")
    ids1 = np.arange(1 << 30, (1 << 30) + 1500, dtype=np.int64)
    items1 = _rand_items(rng, ids1, 48, _usual(1, ids1))
    items1 = np.unique(np.concatenate([items1, _post(0, [17]) | (_rows(w.items[0], 17).astype(U64) << U64(32))]))
    w.file(items1, np.concatenate([[17], ids1]), form="column")
    p = w.group(2)
    assert p.reader.snapshot.info()["dead_union_bytes"] == 0, p.reader.snapshot.info()
    queries = [_old(w, 17, rng)] + [_aimed(rng, w.items[i % 2], 1000, [SHARED, DOUBLE]) for i in range(23)]
    got, st = _both(ctx, p, queries, _legacy(fpx), want=LOW_FILT, want_not=COOP)
    assert got[0][0][0] == 17 and [r[0] for r in got[0]].count(17) == 1


def test_a_clean_group_keeps_k_search_low(tiny):
    """no superseded doc, every column searched: low_wg = 3 is low_wg = 1 -- bit 12 with neither bit 8 nor bit 16, under query_wg 1 and 2"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2592)
    clean = World(Pair, ctx)
    pc, _ = clean.columns(rng, 5, 1500, 48, _usual)
    assert pc.reader.snapshot.info()["dead_union_bytes"] == 0
    queries = [_aimed(rng, clean.items[i % 5], 1000, [SHARED, DOUBLE]) for i in range(24)]
    for query_wg in (1, 2):
        _both(ctx, pc, queries, _legacy(fpx), want=LOW | QUERY_WG | GROUP, want_not=FILTERED | COOP, query_wg=query_wg)


def test_two_packed_groups_behave_as_under_low_wg_2(tiny):
    """the second group's newest column writes doc 17 of the first group again: under groups_wg = 2 the first launch is k_search_low_filt,
    the second k_search_low_next -- bits 13, 12 and 8, never 16: a union bitmap is one group's"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2593)
    w = wg.World(Pair, ctx, snapshot_query_wg=2)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    _more(w, rng, 2, 600, 40, nxt, _usual, again=(17,))
    p = _finish(w, 2)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)], _layout(p)
    queries = [np.concatenate([_rows(w.items[0], 17), _noise(rng, 360)])]
    queries += [_aimed(rng, w.items[i % len(w.items)], 400, [SHARED, DOUBLE][: i % 3]) for i in range(23)]
    got, st = _both(ctx, p, queries, _legacy(fpx), want=GROUPS | LOW_FILT, want_not=COOP, also=[("groups_wg", 2)])
    assert got[0][0][0] == 17 and [d for d, _ in got[0]].count(17) == 1, got[0][:3]


def test_query_wg_1_on_a_filtered_group_is_the_pipelines(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2594)
    w, p, again = _world1(Pair, ctx, rng, 5)
    queries = _world1_queries(rng, w, again, 5, 12)
    _both(ctx, p, queries, _legacy(fpx), want=GROUP, want_not=LOW | FILTERED | QUERY_WG | COOP, query_wg=1)


# ---- 11. hand-back ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def edges(tiny):
    """test_gpu_low_wg_filtered's edge world: 8 columns; HOT8 has 1000 docs in each of them, HOT1 1000 docs in column 0; column 1 holds 3500
    hashes of one doc each, column 3 600 hashes with a list of three docs each; the newest column writes doc 1 of column 0 -- a HOT8
    doc -- again"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2600)
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
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0
    return fpx, ctx, rng, w, p, np.array(singles, dtype=np.uint32), np.array(lists, dtype=np.uint32)


def _records(p, q):
    """the query's LIVE hit records -- what the kernel's array holds: the scores of everything a floor of 1 returns"""
    return sum(s for _, s in p.osnap.search(q, 1 << 20, 1, 0))


def _plain(rng, w, n):
    qs = [_aimed(rng, w.items[i % 8], 300) for i in range(n)]
    return [q[(q != HOT8) & (q != HOT1)] for q in qs]


def _hands_back(fpx, ctx, p, plain, heavy, opts):
    """`plain` is taken; `heavy` -- the same batch with one query too large -- comes back through the pipeline with the oracle's results
    and the path bits cleared, and so does the next batch of that snapshot (the back-off); a fresh snapshot takes the kernel again"""
    got, st = _both(ctx, p, plain, opts)
    for name, value in (("query_wg", 2), ("filt_coop", 1), ("low_wg", 3)):
        ctx.set_option(name, value)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & (LOW | QUERY_WG | FILTERED | COOP) and st_h.path_flags & GROUP, f"not handed back ({st_h.path_flags})"
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, opts.max_results, opts.min_score, opts.min_score_pct)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernel)
        assert not st_n.path_flags & (LOW | QUERY_WG | COOP) and got_n == got, st_n.path_flags
        ctx.set_option("low_wg", 0)
        got_p, st_p = p.reader.search_batch(heavy, opts)
        assert got_p == got_h and _figures(st_p) == _figures(st_h)
        ctx.set_option("query_wg", 2)
        p.finish()                                             # a fresh snapshot of the same segments
    finally:
        for name in ("low_wg", "filt_coop", "query_wg"):
            ctx.set_option(name, -1)
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


def test_records_beyond_the_array_are_handed_back(edges):
    """HOT8 and a few hundred more: 8300 live records, over the array's 8192 (QS_REC_CAP)"""
    fpx, ctx, rng, w, p, singles, lists = edges
    plain = _plain(rng, w, 12)
    heavy = list(plain)
    heavy[5] = np.concatenate([[HOT8], singles[:300]]).astype(np.uint32)
    assert _records(p, heavy[5]) == 8300
    _hands_back(fpx, ctx, p, plain, heavy, _low1(fpx, 100))


def test_tasks_beyond_the_filtered_queue_are_handed_back(edges):
    """a query of 512 hashes with a list each fills the filtered form's task queue (QS_TASKS_FILT) and is taken; one of 513 overflows it --
    1539 records, far from the array's end -- and hands the batch back"""
    fpx, ctx, rng, w, p, singles, lists = edges
    plain = _plain(rng, w, 12)
    plain[3] = lists[:QS_TASKS_FILT].copy()
    heavy = list(plain)
    heavy[5] = lists[: QS_TASKS_FILT + 1].copy()
    assert _records(p, plain[3]) == 3 * QS_TASKS_FILT and _records(p, heavy[5]) == 3 * QS_TASKS_FILT + 3
    _hands_back(fpx, ctx, p, plain, heavy, _low1(fpx, 100))


# ---- 12. the option --------------------------------------------------------------------------------------------------------------------

def test_option_handling(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    monkeypatch.delenv("FPX_LOW_WG", raising=False)
    ctx.set_option("low_wg", -1)
    try:
        assert ctx.get_option("low_wg") == 0                           # the default
        for v in (0, 1, 2, 3):
            ctx.set_option("low_wg", v)
            assert ctx.get_option("low_wg") == v
        monkeypatch.setenv("FPX_LOW_WG", "3")
        ctx.set_option("low_wg", 2)
        assert ctx.get_option("low_wg") == 2
        ctx.set_option("low_wg", -1)
        assert ctx.get_option("low_wg") == 3                           # back to the fallback: the environment
        monkeypatch.delenv("FPX_LOW_WG")
        assert ctx.get_option("low_wg") == 0
    finally:
        ctx.set_option("low_wg", -1)
