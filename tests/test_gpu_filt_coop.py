"""k_search_filt (csrc/fpx_qsearch.hpp, option filt_coop = 1 under query_wg = 2): ONE packed group with superseded docs and/or columns
outside the snapshot, searched by the unfiltered form's rounds -- eight lanes to a line -- behind the group's UNION dead-set bitmap of the
snapshot (bit doc - gmin; built on the device when the snapshot is made under filt_coop = 1, fpx_snapshot_info slot 12).  A kept doc
whose union bit is clear is live; one whose bit is set -- a superseded doc, or its live rewrite in a newer column -- finds its column
and runs that column's exact test.  fpx_stats.path_flags: bit 16 (65536) k_search_filt, with bit 8 (256) the filtered form and bit 6
(64) a query per workgroup; bit 7 (128) where it was part 0 of a snapshot in two parts.

Every comparison goes through wg_harness.both: Pair.check under filt_coop = 1 (results and every query's scanned blocks / docs == the
oracle's, the path bits asserted), then the batch under filt_coop 1 and under 0 -- today's filtered kernel -- compared byte for byte:
results, statistics, per-query blocks / docs, the growth of the scan histograms (nothing unbucketed); and once against query_wg = 0, the
pipeline.  Snapshots are made with FPX_FILT_COOP=1 in the environment (the option's fallback: both() sets and resets the option itself).
The groups are tiny (group_packed = 1, FPX_DIRECT_MIN_ITEMS = 0), one at a time."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import (FILTERED, GROUP, LOW, QS_MAX_HASHES, QUERY_WG, TWO_PARTS, U64,
                        aimed as _aimed, legacy as _legacy, noise as _noise, post as _post, rand_items as _rand_items, rows as _rows)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED, DOUBLE, LINE4 = 0x2BADF00D, 0x37770000, 0x5A5A5A50
COOP = 1 << 16
TAKEN = QUERY_WG | FILTERED | COOP
OPTIONS = ("filt_coop", "low_wg", "hot_wg", "query_wg", "direct_min_items")
FPX_E_INVAL = -4                                     # include/fpx.h
_usual = wg.usual(SHARED, DOUBLE)


def _extra(s, ids):
    """wg.usual, and DOUBLE + 1 -- the next hash value of DOUBLE's line -- a double in every column as well: at nine columns 36 words on
    a line that holds 29, the last eight (DOUBLE + 1's of columns 5 .. 8) in `ext`"""
    return _usual(s, ids) + [(DOUBLE + 1, ids[:2])]


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


def _both(ctx, p, queries, opts, want=TAKEN, want_not=0, also=(), parts=False):
    got, st = wg.both(ctx, p, queries, opts, "filt_coop", 1, clear=COOP, want=want, want_not=want_not, also=[("query_wg", 2)] + list(also))
    ctx.set_option("query_wg", 0)                              # ... and the pipeline
    try:
        got0, st0 = p.reader.search_batch(queries, opts)
    finally:
        ctx.set_option("query_wg", -1)
    assert not st0.path_flags & (QUERY_WG | TWO_PARTS | FILTERED | COOP), st0.path_flags
    assert got0 == got
    assert (st0.scanned_blocks, st0.scanned_docs) == (st.scanned_blocks, st.scanned_docs)
    if not parts:
        assert (st0.probes, st0.hits) == (st.probes, st.hits), ((st0.probes, st0.hits), (st.probes, st.hits))
    return got, st


def _old(w, d, rng, n=500):
    """a query of doc d's hashes in the OLDEST column that has it, and noise"""
    return np.concatenate([_rows(next(it for it in w.items if len(_rows(it, d))), d), _noise(rng, n)])


HIGH = dict(max_results=100, min_score=3, min_score_pct=0)


# ---- 1. every kind of word superseded -----------------------------------------------------------------------------------------------

def _world1(Pair, ctx, rng, cols):
    """the newest column writes again, with their SAME hashes: doc 17 of column 0 (a plain inline word), doc per + 1 (the first word of
    column 1's doubles), doc 2 (the second word of column 0's), doc 2 per + 3 (in column 2's list of 4: a list's head), doc 3 per + 41 (in
    column 3's list of 70: read on by the wave) and, at nine columns, doc 6 per + 1 (DOUBLE + 1's words of column 6: in `ext`)"""
    per = 1500
    again = [17, per + 1, 2, 2 * per + 3, 3 * per + 41] + ([6 * per + 1] if cols == 9 else [])
    w = World(Pair, ctx)
    p, _ = w.columns(rng, cols, per, 48, _extra, again={d: None for d in again})
    return w, p, again


def _world1_queries(rng, w, again, cols, n=30):
    queries = [_old(w, d, rng) for d in again]
    return queries + [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE, DOUBLE + 1][: i % 4]) for i in range(n - len(queries))]


@pytest.mark.parametrize("cols", [5, 9])
def test_every_kind_of_word_superseded(tiny, cols):
    """each rewritten doc is returned exactly once -- the newest column's posting, whose union bit is set although it is live there --,
    and scanned_docs is the oracle's (Pair.check): the superseded postings are counted before they are dropped"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2300 + cols)
    w, p, again = _world1(Pair, ctx, rng, cols)
    assert p.reader.snapshot.info()["dead_union_bytes"] == 4 * (((cols * 1500 - 1) >> 5) + 1), p.reader.snapshot.info()
    queries = _world1_queries(rng, w, again, cols)
    for opts in (fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0)):
        got, st = _both(ctx, p, queries, opts)
        for i, d in enumerate(again):
            assert got[i] and got[i][0][0] == d and [r[0] for r in got[i]].count(d) == 1, (d, got[i][:4])


# ---- 2. a whole line superseded -----------------------------------------------------------------------------------------------------

def test_a_whole_line_superseded(tiny):
    """nine columns (lines of four hash values): the four hash values of ONE line each have a doc in the seven oldest columns -- 28 inline
    words, every one of them the line's --, and the newest column writes all seven docs again, with other hashes.  A query with all four
    hashes: all eight lanes of a group have dead words in that line; an old posting counted would give its doc a score of 4"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2320)
    per = 1500
    w = World(Pair, ctx)
    gone = [s * per + 11 for s in range(7)]
    fresh = {d: rng.integers(0, 1 << 32, 48, dtype=U64).tolist() for d in gone}
    p, _ = w.columns(rng, 9, per, 48, lambda s, ids: _usual(s, ids) + ([(LINE4 + k, ids[10:11]) for k in range(4)] if s < 7 else []), again=fresh)
    line = np.arange(LINE4, LINE4 + 4, dtype=np.uint32)
    queries = [np.concatenate([line, _noise(rng, 900)]), np.concatenate([line, line, _rows(w.items[0], 11), _noise(rng, 500)])]
    queries += [np.concatenate([np.asarray(fresh[d], dtype=np.uint32), line, _noise(rng, 600)]) for d in gone]
    queries += [_aimed(rng, w.items[i % 9], 1000, [SHARED, DOUBLE, LINE4 + i % 4]) for i in range(16)]
    got, st = _both(ctx, p, queries, fpx.SearchOptions(**HIGH))
    assert not any(r[0] in gone for r in got[0] + got[1]), (got[0][:4], got[1][:4])
    for i, d in enumerate(gone):
        assert got[2 + i][0] == (d, 48) and [r[0] for r in got[2 + i]].count(d) == 1, (d, got[2 + i][:3])
    _both(ctx, p, queries, fpx.http_options())


# ---- 3. the bitmap's edges ----------------------------------------------------------------------------------------------------------

def _world3(Pair, ctx, rng, cols, first):
    """a memory segment writes again, with new hashes, the group's docs gmin, gmin + 31, gmin + 32 and its largest id"""
    per = 1500
    w = World(Pair, ctx)
    w.columns(rng, cols, per, 48, _usual, first=first)
    last = first + cols * per - 1
    gone = [first, first + 31, first + 32, last]
    w.memory(_rand_items(rng, gone, 48), gone)
    return w, w.finish(), gone, last


@pytest.mark.parametrize("cols", [5, 9])
@pytest.mark.parametrize("high", [False, True], ids=["from_1", "to_0xFFFFFFFF"])
def test_bitmap_edges(tiny, cols, high):
    """superseded: the first bit of the bitmap, the last bit of its first word, the first of its second, its last bit; a live doc next
    to each.  Ids from 1, and ids up to 0xFFFFFFFF (gmin + word must not overflow)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2330 + cols + high)
    first = ((1 << 32) - cols * 1500) if high else 1
    w, p, gone, last = _world3(Pair, ctx, rng, cols, first)
    assert not high or (first >= 0xFFFF0000 and last == 0xFFFFFFFF)
    info = p.reader.snapshot.info()
    assert info["memory"] == 1 and info["dead_union_bytes"] == 4 * (((last - first) >> 5) + 1), info
    near = [first + 1, first + 30, first + 33, last - 1]
    queries = [_old(w, d, rng) for d in gone] + [_old(w, d, rng) for d in near]
    queries += [np.concatenate([_rows(w.items[-1], d), _noise(rng, 500)]) for d in gone]         # (the new hashes)
    queries += [_aimed(rng, w.items[i % cols], 1000, [SHARED, DOUBLE]) for i in range(12)]
    got, st = _both(ctx, p, queries, fpx.http_options())
    for i, d in enumerate(gone):
        assert d not in [r[0] for r in got[i]], (d, got[i][:3])
        assert got[8 + i][0] == (d, 48), (d, got[8 + i][:2])
    for i, d in enumerate(near):
        assert got[4 + i] and got[4 + i][0][0] == d, (d, got[4 + i][:2])


# ---- 4. memory segments: tombstones, re-inserts with new hashes, deletes ----------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_memory_segments_supersede_group_docs(tiny, cols):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2340 + cols)
    per = 1500
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, cols, per, 48, _usual)
    again = [17, 2 * per + 3, 3 * per + 41]                    # (a plain doc, one in a list of 4, one in a list of 70)
    deleted = [2, per + 1, 4 * per + 9]
    for m in range(3):
        ids = list(range(nxt, nxt + 50)) + (again if m == 1 else [])
        w.memory(_rand_items(rng, ids, 40), sorted(ids))
        nxt += 50
    w.changes([("delete", d) for d in deleted] + [("insert", nxt, rng.integers(0, 1 << 32, 30).tolist())])
    p = w.finish()
    assert p.reader.snapshot.info()["memory"] == 4 and p.reader.snapshot.info()["dead_union_bytes"] != 0
    queries = [_old(w, d, rng) for d in again + deleted]
    queries += [np.concatenate([_rows(w.items[cols + 1], d), _noise(rng, 300)]) for d in again]  # (the new hashes)
    queries += [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(18)]
    for opts in (fpx.http_options(), fpx.SearchOptions(**HIGH)):
        got, st = _both(ctx, p, queries, opts)
        for i, d in enumerate(again + deleted):
            assert d not in [r[0] for r in got[i]], (d, got[i][:3])
        for i, d in enumerate(again):
            assert got[6 + i][0] == (d, 40), (d, got[6 + i][:2])
        assert not any(r[0] in deleted for g in got for r in g), "a deleted doc was returned"


# ---- 5. two parts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_two_parts(tiny, cols):
    """checkpoints in blocks next to the group, one tombstoning a group doc and one writing one again: part 0 is the filtered group, whose
    dead sets hold part 1's docs -- bits 7, 8 and 16"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2350 + cols)
    per = 1500
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, cols, per, 48, _usual)
    for s in range(2):
        ids, alive = list(range(nxt, nxt + 600)), [1] * 600
        items = _rand_items(rng, ids, 40, [(SHARED, ids[:7])])
        if s == 0:
            ids.insert(0, 5); alive.insert(0, 0)                   # doc 5 of the group: a tombstone
        else:                                                      # ... and doc per + 9 written again, with its own hashes
            items = np.unique(np.concatenate([items, _post(0, [per + 9]) | (_rows(w.items[1], per + 9).astype(U64) << U64(32))]))
            ids.insert(0, per + 9); alive.insert(0, 1)
        w.file(items, ids, form="blocks", alive=np.array(alive, dtype=np.uint8))
        nxt += 600
    p = w.finish()
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0, p.reader.snapshot.info()
    queries = [_old(w, 5, rng), _old(w, per + 9, rng)]
    queries += [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(30)]
    for opts in (fpx.http_options(), fpx.SearchOptions(max_results=60, min_score=4, min_score_pct=30)):
        got, st = _both(ctx, p, queries, opts, want=TAKEN | TWO_PARTS, parts=True)
        assert 5 not in [r[0] for r in got[0]] and got[1][0][0] == per + 9 and [r[0] for r in got[1]].count(per + 9) == 1, (got[0][:2], got[1][:2])


# ---- 6. columns outside the snapshot ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
@pytest.mark.parametrize("dead", [False, True])
def test_masked_columns_after_a_merge_without_regroup(tiny, cols, dead):
    """the two oldest columns merged away (a segment of its own next to the group, no regroup): their words -- SHARED a double and a
    list of 3, DOUBLE doubles -- share lines with the active columns' and give nothing.  Without a dead set anywhere there is no bitmap
    and no test, and the kernel is k_search_filt all the same; with one in an active column both masks work together"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2360 + cols + dead)
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
    for opts in (fpx.http_options(), fpx.SearchOptions(max_results=80, **{k: v for k, v in HIGH.items() if k != "max_results"})):
        got, st = _both(ctx, q.p, queries, opts, want=TAKEN | TWO_PARTS, parts=True)
    assert got[0][0][0] == 17 and got[1][0][0] == per + 500 and [r[0] for r in got[0]].count(17) == 1     # (found in the merged segment, once)
    assert got[4][0][0] == 2 * per + 2
    for i, d in ((2, 2 * per + 1), (3, 3 * per + 41)):
        assert (d not in [r[0] for r in got[i]]) if dead else got[i][0][0] == d, (d, got[i][:3])


# ---- 7. fallbacks keep today's kernel -----------------------------------------------------------------------------------------------

def test_a_snapshot_made_under_0_keeps_todays_kernel(tiny, monkeypatch):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2370)
    monkeypatch.setenv("FPX_FILT_COOP", "0")
    w, p, again = _world1(Pair, ctx, rng, 5)
    assert p.reader.snapshot.info()["dead_union_bytes"] == 0
    queries = _world1_queries(rng, w, again, 5, 24)
    _both(ctx, p, queries, fpx.http_options(), want=QUERY_WG | FILTERED, want_not=COOP)
    monkeypatch.setenv("FPX_FILT_COOP", "1")
    w.finish()                                                 # (a fresh snapshot under 1: taken)
    assert p.reader.snapshot.info()["dead_union_bytes"] != 0
    _both(ctx, p, queries, fpx.http_options())


def test_an_id_range_beyond_2_to_the_29_keeps_todays_kernel(tiny):
    """two columns, ids from 1 and from 2^30; the second writes doc 17 of the first again: no bitmap over a range that wide"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2371)
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
    got, st = _both(ctx, p, queries, fpx.http_options(), want=QUERY_WG | FILTERED, want_not=COOP)
    assert got[0][0][0] == 17 and [r[0] for r in got[0]].count(17) == 1


def test_a_low_floor_and_a_clean_group_keep_their_kernels(tiny):
    """a batch with a low-floor query under low_wg = 2 is k_search_low_filt's (bits 12 and 8, not 16); a CLEAN group under filt_coop = 1
    is the unfiltered kernel's (neither bit 8 nor bit 16)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2372)
    w, p, again = _world1(Pair, ctx, rng, 5)
    queries = _world1_queries(rng, w, again, 5, 24)
    _both(ctx, p, queries, _legacy(fpx), want=QUERY_WG | FILTERED | LOW, want_not=COOP, also=[("low_wg", 2)])
    clean = World(Pair, ctx)
    pc, _ = clean.columns(rng, 5, 1500, 48, _usual)
    assert pc.reader.snapshot.info()["dead_union_bytes"] == 0
    queries = [_aimed(rng, clean.items[i % 5], 1000, [SHARED, DOUBLE]) for i in range(24)]
    _both(ctx, pc, queries, fpx.http_options(), want=QUERY_WG | GROUP, want_not=FILTERED | COOP)


# ---- 8. query shapes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [5, 9])
def test_query_shapes(tiny, cols):
    """1, 255, 256, 257, 1025 and 4096 hashes, duplicates inside a query: lanes without a probe in a round, the rolling window beyond
    1024 hashes"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2380 + cols)
    w, p, again = _world1(Pair, ctx, rng, cols)
    own = _rows(w.items[0], 17)
    special = np.array([SHARED, DOUBLE, DOUBLE + 1, SHARED], dtype=np.uint32)
    shapes = [own[:1]]
    for n in (255, 256, 257, 1025, QS_MAX_HASHES):
        q = np.concatenate([own, own[:9], special, _noise(rng, n - len(own) - 9 - len(special))])
        rng.shuffle(q)
        shapes.append(q)
    shapes += [np.full(500, int(own[0]), dtype=np.uint32), np.concatenate([_old(w, 3 * 1500 + 41, rng, 2000), special])]
    assert [len(x) for x in shapes[:6]] == [1, 255, 256, 257, 1025, 4096]
    got, st = _both(ctx, p, shapes, fpx.SearchOptions(**HIGH))
    assert all(g[0] == (17, len(own)) for g in got[1:6]), [g[:1] for g in got[1:6]]      # (a duplicate is no probe)


# ---- 9. hand-back -------------------------------------------------------------------------------------------------------------------

def test_hot_hashes_are_handed_back(tiny):
    """a query of twelve hashes of 1500 docs each outgrows the LDS records: k_search_filt hands the batch back (CTR_BINFAIL) as the
    filtered k_search_query does -- bits 6, 8 and 16 clear, the pipeline's answers"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2390)
    per = 4000
    hots = [0x40000000 + 977 * k for k in range(12)]
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 3, per, 48, lambda s, ids: [(k, ids[:1500]) for k in hots[s::3]], again={11: None})
    plain = [_old(w, 11, rng)] + [_aimed(rng, w.items[i % 3], 1000) for i in range(15)]
    plain = [q[~np.isin(q, hots)] for q in plain]
    _both(ctx, p, plain, fpx.http_options())
    heavy = list(plain)
    heavy[5] = np.concatenate([plain[5][:900], np.array(hots, dtype=np.uint32)])
    ctx.set_option("query_wg", 2)
    try:
        got_h, st_h = p.reader.search_batch(heavy, fpx.http_options())
    finally:
        ctx.set_option("query_wg", -1)
    assert not st_h.path_flags & (QUERY_WG | FILTERED | COOP), st_h.path_flags
    for qq, g in zip(heavy, got_h):
        assert g == p.osnap.search(qq, 40, None, 10)


# ---- 10. the snapshot's bookkeeping -------------------------------------------------------------------------------------------------

def test_snapshot_bookkeeping(tiny):
    """two snapshots in a row over unchanged segments report the same bitmap and both search correctly, the second after the first is
    released; a publish that adds a dead doc gives a snapshot that drops it, while the older snapshot still returns it"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(2400)
    w, p, gone, last = _world3(Pair, ctx, rng, 5, 1)
    want_bytes = 4 * (((last - 1) >> 5) + 1)
    queries = [_old(w, d, rng) for d in gone + [40, 41]] + [_aimed(rng, w.items[i % 5], 1000, [SHARED, DOUBLE]) for i in range(18)]
    r1 = p.reader
    assert r1.snapshot.info()["dead_union_bytes"] == want_bytes
    got1, _ = _both(ctx, p, queries, fpx.http_options())
    w.finish()
    assert p.reader is not r1 and p.reader.snapshot.info()["dead_union_bytes"] == want_bytes
    r1.snapshot.release()
    del r1
    gc.collect()
    got2, _ = _both(ctx, p, queries, fpx.http_options())
    assert got2 == got1 and got1[4][0][0] == 40
    r2, o2 = p.reader, p.osnap
    w.changes([("delete", 40)])
    w.finish()
    assert p.reader.snapshot.info()["dead_union_bytes"] == want_bytes
    got3, _ = _both(ctx, p, queries, fpx.http_options())
    assert 40 not in [r[0] for r in got3[4]] and got3[5][0][0] == 41
    p.reader, p.osnap = r2, o2                                 # (the older snapshot: its own bitmap)
    got4, _ = _both(ctx, p, queries, fpx.http_options())
    assert got4 == got1


# ---- 11. fresh memory ---------------------------------------------------------------------------------------------------------------

def test_fresh_memory_holds_anything(env):
    """world 1 once more in a child process under FPX_POISON=1: every fresh device allocation filled with 0xCD -- the bitmap is zeroed
    before the columns' lists are scattered into it"""
    if os.environ.get("FPX_VARIANT_CHILD") == "1":
        return
    env[3].trim()                                              # (the line buffer this process keeps for its next group: the child's to take)
    gc.collect()
    e = dict(os.environ, FPX_VARIANT_CHILD="1", FPX_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_filt_coop.py::test_every_kind_of_word_superseded[5]"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-1000:]


# ---- 12. the option -----------------------------------------------------------------------------------------------------------------

def test_option_handling(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    monkeypatch.delenv("FPX_FILT_COOP", raising=False)
    ctx.set_option("filt_coop", -1)
    try:
        assert ctx.get_option("filt_coop") == 0                        # the default
        for v in (0, 1):
            ctx.set_option("filt_coop", v)
            assert ctx.get_option("filt_coop") == v
        with pytest.raises(fpx.FpxError) as refused:
            ctx.set_option("filt_coop", 2)
        assert refused.value.status == FPX_E_INVAL and "filt_coop is 0 or 1" in str(refused.value), refused.value
        assert ctx.get_option("filt_coop") == 1                        # a refused value changes nothing
        monkeypatch.setenv("FPX_FILT_COOP", "1")
        ctx.set_option("filt_coop", 0)
        assert ctx.get_option("filt_coop") == 0
        ctx.set_option("filt_coop", -1)
        assert ctx.get_option("filt_coop") == 1                        # back to the fallback: the environment
        monkeypatch.delenv("FPX_FILT_COOP")
        assert ctx.get_option("filt_coop") == 0
    finally:
        ctx.set_option("filt_coop", -1)
