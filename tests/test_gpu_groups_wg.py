"""Option groups_wg = 1 (csrc/fpx_qsearch.hpp: k_search_next): a snapshot of SEVERAL packed groups -- an index with more dense segments
than one group's 16 columns, merge results that met and formed a group of their own -- is walked group by group a query per workgroup:
k_search_query over the first group (with the memory segments' table), k_search_next over the others, whose hand-over CHAINS behind the
launch before; one k_finish.  fpx_stats.path_flags: bit 13 (8192) several groups were walked that way, with bit 6 (64) a query per
workgroup and bit 2 (4) a group; bit 8 (256) when any group is filtered, bit 7 (128) two parts, bit 1 (2) the shared candidate list.

A second group is made the way test_gpu_query_wg.py::test_a_second_group_next_to_the_large_one makes one: segments filed as direct-
addressed candidates AFTER the first snapshot meet in a group of their own at the next.  Every case goes through wg_harness.both():
Pair.check under groups_wg = 1 (results and every query's scanned blocks / docs == the oracle's) with the path bits asserted, then the
batch under 1 and under 0 compared: results, scanned_blocks, scanned_docs, probes, hits, algorithmic_bytes, per-query blocks / docs and
the growth of the scan histograms.  Each with http_options() and once with an explicit floor.  The worlds are a few thousand docs x 40
hashes.  Snapshots are made under groups_wg = 1 (_finish): the option also decides, when a snapshot is made, whether its groups are
split over two parts -- one made under 0 keeps the smaller groups in part 1 whatever the option says later.  On a library without the
option the `tiny` fixture's set_option("groups_wg", ...) raises: every test here fails there."""
import numpy as np
import pytest

import wg_harness as wg
from wg_harness import (FILTERED, GROUP, LOW, QS_REC_CAP, QUERY_WG, SECOND_TRIP, TWO_PARTS, U64,
                        aimed as _aimed, legacy as _legacy, noise as _noise, post as _post, rand_items as _rand_items, rows as _rows)

pytestmark = pytest.mark.gpu

GROUPS = 8192                       # fpx_stats.path_flags bit 13
TAKEN = GROUPS | QUERY_WG | GROUP
OPTIONS = ("groups_wg", "query_wg", "low_wg", "hot_wg", "direct_min_items")
SHARED, DOUBLE, HAND, HOTB = 0x2BADF00D, 0x37770000, 0x61000000, 0x4BCDEF01
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


def _more(w, rng, cols, per, nh, first, extra=lambda s, ids: [], block_size=512, again=()):
    """`cols` more columns of `per` docs x `nh` hashes from doc `first`, filed as candidates behind a snapshot: they meet in a group of their
    own at the next one.  again: docs of older segments that the newest of these columns writes again, with their own hashes.
    -> the first free doc"""
    for s in range(cols):
        ids = np.arange(first + s * per, first + (s + 1) * per, dtype=np.int64)
        items = _rand_items(rng, ids, nh, extra(s, ids))
        if s == cols - 1 and again:
            for d in again:
                old = next(it for it in w.items if len(_rows(it, d)))
                items = np.unique(np.concatenate([items, _post(0, [d]) | (_rows(old, d).astype(U64) << U64(32))]))
            ids = np.array(sorted(list(ids) + list(again)), dtype=np.int64)
        w.file(items, ids, form="column", block_size=block_size)
    return first + cols * per


def _finish(w, groups_wg=None):
    """a snapshot, made under groups_wg where given (the value in force when its two parts are chosen)"""
    if groups_wg is None:
        return w.finish()
    w.ctx.set_option("groups_wg", groups_wg)
    try:
        return w.finish()
    finally:
        w.ctx.set_option("groups_wg", -1)


def _layout(p):
    """[(columns, line_columns, packed)] of the file segments' groups, in segment order (group_info(): a group's column 0 opens it)"""
    out = []
    for g in p.gpu_segs[: len(p.orc_file)]:
        i = g.group_info()
        if i is None:
            continue
        if i["column"] == 0:
            out.append([i["columns"], i["line_columns"], i["packed"], 0])
        out[-1][3] += 1
    assert all(c == n for c, _, _, n in out), out
    return [(c, l, k) for c, l, k, _ in out]


def _both(ctx, p, queries, opts, want=TAKEN, want_not=0, also=()):
    return wg.both(ctx, p, queries, opts, "groups_wg", 1, clear=GROUPS, want=want, want_not=want_not, also=also, compare=wg.WITH_BYTES)


def _twice(fpx, ctx, p, queries, **kw):
    """under http_options() and under an explicit floor, relative cut and limit -> the first's results"""
    got, _ = _both(ctx, p, queries, fpx.http_options(), **kw)
    _both(ctx, p, queries, fpx.SearchOptions(max_results=80, min_score=4, min_score_pct=30), **kw)
    return got


def _queries(rng, w, n, qlen=400):
    """queries of 400 hashes (a default floor of 20) aimed at docs of the world's segments in turn"""
    return [_aimed(rng, w.items[i % len(w.items)], qlen, [SHARED, DOUBLE][: i % 3]) for i in range(n)]


def _two_groups(Pair, ctx, rng, cols0=4, cols1=2, per0=800, per1=600, extra1=lambda s, ids: [], **kw):
    w = wg.World(Pair, ctx, **kw)
    _, nxt = w.columns(rng, cols0, per0, 40, _usual)
    return w, nxt, _more(w, rng, cols1, per1, 40, nxt, extra1)


# ---- 1. two clean groups, nothing else ------------------------------------------------------------------------------------------------

def test_two_clean_groups_and_nothing_else(tiny):
    """5 + 2 columns, both of 8-column lines: no parts (nothing is left for a part 1), bits 13, 6 and 2"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1800)
    w, end0, _ = _two_groups(Pair, ctx, rng, 5, 2, 1200, 900, lambda s, ids: [(SHARED, ids[:11])])
    p = _finish(w, 1)
    assert _layout(p) == [(5, 8, 1), (2, 8, 1)], _layout(p)
    info = p.reader.snapshot.info()
    assert info["groups"] == 2 and info["packed_groups"] == 2, info
    got = _twice(fpx, ctx, p, _queries(rng, w, 28), want_not=TWO_PARTS | FILTERED)
    best = [g[0][0] for g in got if g]
    assert sum(1 for d in best if d < end0) >= 3 and sum(1 for d in best if d >= end0) >= 3, best
    # off by default: the pipeline
    _, st = p.reader.search_batch(_queries(rng, w, 8), fpx.http_options())
    assert not st.path_flags & (GROUPS | QUERY_WG) and st.path_flags & GROUP, st.path_flags


# ---- 2. mixed line widths ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [(9, 3), (3, 9)])
def test_mixed_line_widths(tiny, cols):
    """a group of 9 columns (lines of 4 hash values) and one of 3 (lines of 8), in both orders: NS is each launch's own"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1810 + cols[0])
    w, end0, _ = _two_groups(Pair, ctx, rng, cols[0], cols[1], 500, 500, _usual)
    p = _finish(w, 1)
    assert _layout(p) == [(c, 8 if c <= 8 else 16, 1) for c in cols], _layout(p)
    got = _twice(fpx, ctx, p, _queries(rng, w, 24), want_not=TWO_PARTS)
    best = [g[0][0] for g in got if g]
    assert sum(1 for d in best if d < end0) >= 3 and sum(1 for d in best if d >= end0) >= 3, best


# ---- 3. three groups ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["finish", "block_size"])
def test_three_groups(tiny, how):
    """the third group by a third snapshot, or -- a group holds segments of ONE block size -- by two segments of 1024-byte blocks filed with
    the second group's: the groups' algorithmic bytes (512 and 1024 a block) add up to the pipeline's"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1820 + len(how))
    w, _, nxt = _two_groups(Pair, ctx, rng, 4, 2, 600, 600, _usual)
    if how == "finish":
        p = w.finish()
        assert _layout(p) == [(4, 8, 1), (2, 8, 1)], _layout(p)
        _more(w, rng, 2, 600, 40, nxt, _usual)
        p = _finish(w, 1)                                      # (the third snapshot)
    else:
        _more(w, rng, 2, 600, 40, nxt, _usual, block_size=1024)
        p = _finish(w, 1)                                      # (the second snapshot: the block sizes kept the four apart)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1), (2, 8, 1)], _layout(p)
    assert p.reader.snapshot.info()["packed_groups"] == 3
    got = _twice(fpx, ctx, p, _queries(rng, w, 24), want_not=TWO_PARTS)
    assert len({min(2, max(0, (g[0][0] - 1201) // 1200)) for g in got if g}) == 3        # (best docs in all three groups)


# ---- 4. memory segments next to two groups --------------------------------------------------------------------------------------------

def test_memory_segments_next_to_two_groups(tiny):
    """the groups' docs start at 1000; a memory segment holds docs 5 .. 44 -- below every group's gmin: their records wrap in the first
    launch, which alone has the memory table -- and one of them is found by a query that finds nothing else"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1830)
    w = wg.World(Pair, ctx)
    _, nxt = w.columns(rng, 4, 800, 40, _usual, first=1000)
    _more(w, rng, 2, 600, 40, nxt, _usual)
    ids = np.arange(5, 45)
    w.memory(_rand_items(rng, ids, 40), ids)
    p = _finish(w, 1)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)] and p.reader.snapshot.info()["memory"] == 1
    mem = w.items[-1]
    queries = [np.concatenate([_rows(mem, 5), _noise(rng, 360)]), np.concatenate([_rows(mem, 20), _noise(rng, 360)])] + _queries(rng, w, 22)
    got = _twice(fpx, ctx, p, queries, want_not=TWO_PARTS)
    assert got[0][0][0] == 5 and [d for d, _ in got[1]] == [20], (got[0][:2], got[1])
    assert any(g and 5 <= g[0][0] < 45 for g in got[2:]) and any(g and g[0][0] >= nxt for g in got[2:])


# ---- 5. the chained hand-over, case by case ---------------------------------------------------------------------------------------------

# candidates of a query per group: three hashes list the same k docs of the group's first column, which so reach a floor of 3
CASES = [(2, 2, 0), (3, 2, 0), (6, 1, 0), (0, 3, 0), (3, 0, 0), (1, 40, 0), (1, 1, 3)]
IN_SLOTS = (0, 3, 4)                # the cases that never leave the queries' own four slots


def _hand(c, j):
    return HAND + 7919 * (3 * c + j)


def _hand_extra(gi):
    return lambda s, ids: [(_hand(c, j), ids[50 * c: 50 * c + k[gi]]) for c, k in enumerate(CASES) for j in range(3) if s == 0 and k[gi]]


@pytest.fixture
def handover(tiny):
    """three groups (3 + 2 + 2 columns of 600 docs); case c's docs are ids[50 c : 50 c + k] of each group's first column"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1840)
    w = wg.World(Pair, ctx)
    firsts = [1]
    _, nxt = w.columns(rng, 3, 600, 40, _hand_extra(0))
    firsts.append(nxt)
    nxt = _more(w, rng, 2, 600, 40, nxt, _hand_extra(1))
    w.finish()
    firsts.append(nxt)
    _more(w, rng, 2, 600, 40, nxt, _hand_extra(2))
    p = _finish(w, 1)
    assert _layout(p) == [(3, 8, 1), (2, 8, 1), (2, 8, 1)], _layout(p)

    def query(c):                                              # (50 hashes: a default floor of 3)
        q = np.concatenate([np.array([_hand(c, j) for j in range(3)], dtype=np.uint32), _noise(rng, 47)])
        rng.shuffle(q)
        return q

    def docs(c):
        return sorted(firsts[gi] + 50 * c + i for gi in range(3) for i in range(CASES[c][gi]))

    return fpx, ctx, p, query, docs


def test_the_chained_hand_over(handover):
    """2 + 2: the slots fill exactly; 3 + 2: the earlier slots move to the shared list; 6 + 1: the first launch overflowed already; 0 + 3;
    3 + 0; 1 + 40: more than the LDS buffer's 32 in the later group; 1 + 1 + 3 over three groups.  Every query's docs, each with a score
    of 3; the shared list was used (bit 1) -- and is not by a batch of 2 + 2, 0 + 3 and 3 + 0 alone"""
    fpx, ctx, p, query, docs = handover
    exact = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    order = [c for c in range(len(CASES)) for _ in range(3)]
    queries = [query(c) for c in order]
    _both(ctx, p, queries, fpx.http_options(), want=TAKEN | SECOND_TRIP)
    got, _ = _both(ctx, p, queries, exact, want=TAKEN | SECOND_TRIP)
    for c, g in zip(order, got):
        assert sorted(d for d, _ in g) == docs(c) and all(s == 3 for _, s in g), (CASES[c], g[:8])
    order = [c for c in IN_SLOTS for _ in range(4)]
    queries = [query(c) for c in order]
    _both(ctx, p, queries, fpx.http_options(), want_not=SECOND_TRIP)
    got, _ = _both(ctx, p, queries, exact, want_not=SECOND_TRIP)
    for c, g in zip(order, got):
        assert sorted(d for d, _ in g) == docs(c), (CASES[c], g[:8])


# ---- 6. filtered groups -------------------------------------------------------------------------------------------------------------

def test_a_dead_set_in_the_first_group_only(tiny):
    """the second group's newest column writes doc 17 of the first group again: group 0 has a dead set, group 1 none -- the first launch is
    the filtered k_search_query, the second the plain k_search_next.  Under query_wg = 2 only"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1850)
    w = wg.World(Pair, ctx, snapshot_query_wg=2)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    _more(w, rng, 2, 600, 40, nxt, _usual, again=(17,))
    p = _finish(w, 1)
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)], _layout(p)
    queries = [np.concatenate([_rows(w.items[0], 17), _noise(rng, 360)])] + _queries(rng, w, 23)
    got = _twice(fpx, ctx, p, queries, want=TAKEN | FILTERED, want_not=TWO_PARTS, also=(("query_wg", 2),))
    assert got[0][0][0] == 17 and [d for d, _ in got[0]].count(17) == 1, got[0][:3]
    _twice(fpx, ctx, p, queries, want=GROUP, want_not=GROUPS | QUERY_WG | FILTERED, also=(("query_wg", 1),))


def test_a_column_merged_away_from_the_first_group(tiny):
    """the first group's two oldest columns are merged into a segment of its own (no regroup): the group keeps two columns outside the
    snapshot -- `active` is not all --, the merged segment is part 1 of a snapshot made under groups_wg = 1, query_wg = 2, both groups part 0"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1860)
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
    _finish(q, 1)
    assert q.p.reader.snapshot.info()["groups"] == 2
    queries = [np.concatenate([_rows(w.items[0], 17), _noise(rng, 360)])] + _queries(rng, w, 23)
    got = _twice(fpx, ctx, q.p, queries, want=TAKEN | FILTERED | TWO_PARTS, also=(("query_wg", 2),))
    assert got[0][0][0] == 17 and [d for d, _ in got[0]].count(17) == 1, got[0][:3]       # (found in the merged segment, once)


# ---- 7. two parts -------------------------------------------------------------------------------------------------------------------

def test_two_parts(tiny):
    """two groups, a checkpoint in blocks and a memory segment.  The snapshot made under groups_wg = 1: part 0 is BOTH groups (and the
    memory segment), bits 13 and 7 -- the snapshot has two groups and more than one was walked a query per workgroup, so part 1 holds
    none.  The same segments in a snapshot made under 0: part 0 is the larger group alone, bit 13 clear, the same results"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1870)
    w, _, nxt = _two_groups(Pair, ctx, rng, 4, 2, 800, 600, _usual)
    ids = np.arange(nxt, nxt + 500)
    w.file(_rand_items(rng, ids, 40, [(SHARED, ids[:7])]), ids, form="blocks")
    ids = np.arange(nxt + 500, nxt + 540)
    w.memory(_rand_items(rng, ids, 40), ids)
    p = _finish(w, 1)
    info = p.reader.snapshot.info()
    assert _layout(p) == [(4, 8, 1), (2, 8, 1)] and info["groups"] == 2 and info["memory"] == 1 and not p.gpu_segs[6].grouped, info
    queries = _queries(rng, w, 32)
    got = _twice(fpx, ctx, p, queries, want=TAKEN | TWO_PARTS)
    assert len({(g[0][0] > 3200) + (g[0][0] >= nxt) + (g[0][0] >= nxt + 500) for g in got if g}) == 4      # (best docs in both groups, the checkpoint, the memory segment)
    p = _finish(w, 0)
    ctx.set_option("groups_wg", 1)
    try:
        got0, st0 = p.reader.search_batch(queries, fpx.http_options())
    finally:
        ctx.set_option("groups_wg", -1)
    assert st0.path_flags & (TWO_PARTS | QUERY_WG) == TWO_PARTS | QUERY_WG and not st0.path_flags & GROUPS, st0.path_flags
    assert got0 == got


# ---- 8. what stays off the path -------------------------------------------------------------------------------------------------------

def test_a_legacy_query_keeps_the_batch_off(tiny):
    """one query with a floor of 1 among the batch's, under low_wg = 1: the pipeline's, whatever low_wg says"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1880)
    w, _, _ = _two_groups(Pair, ctx, rng)
    p = _finish(w, 1)
    queries = _queries(rng, w, 12)
    opts = [fpx.http_options()] * 12
    opts[3] = _legacy(fpx)
    _both(ctx, p, queries, opts, want=GROUP, want_not=GROUPS | QUERY_WG | LOW, also=(("low_wg", 1),))
    _both(ctx, p, queries, fpx.http_options(), also=(("low_wg", 1),))         # (without it: taken)


def test_a_group_in_directory_and_words_form_among_them(tiny):
    """the second group in directory + words form: not walked this way -- the packed group alone is part 0 of the snapshot's two parts"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1890)
    w = wg.World(Pair, ctx)
    _, nxt = w.columns(rng, 4, 800, 40, _usual)
    ctx.set_option("group_packed", 0)
    _more(w, rng, 2, 600, 40, nxt, _usual)
    p = _finish(w, 1)
    assert _layout(p) == [(4, 8, 1), (2, 8, 0)], _layout(p)
    _twice(fpx, ctx, p, _queries(rng, w, 16), want=GROUP, want_not=GROUPS)


# (QS_MAX_GROUPS + 1 groups: a packed group's lines span the whole hash space whatever it holds -- 69 GB of address space and a good part of
# it backed --, and the fifth group of a world no longer finds room on one GPU: such a world does not build, the case is left out)


# ---- 9. a hand-back from the second launch --------------------------------------------------------------------------------------------

def test_records_beyond_the_array_in_the_second_group_are_handed_back(tiny):
    """five hashes with 1000 docs each in both columns of the SECOND group: 10 000 hit records there, over the array's 8192, nothing in the
    first.  The batch comes back right, by the pipeline; the snapshot's next batch stays there (the back-off); a fresh snapshot is taken"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1910)
    hot = np.array([HOTB + 7919 * k for k in range(5)], dtype=np.uint32)
    w, _, _ = _two_groups(Pair, ctx, rng, 4, 2, 800, 1200, lambda s, ids: [(int(h), ids[:1000]) for h in hot])
    p = _finish(w, 1)
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    plain = [q[~np.isin(q, hot)] for q in _queries(rng, w, 12)]      # (a doc of the second group's first thousand has the five among its own)
    heavy = list(plain)
    heavy[5] = np.concatenate([hot, _noise(rng, 60)])
    assert sum(s for _, s in p.osnap.search(heavy[5], 1 << 20, 1, 0)) > QS_REC_CAP
    got, _ = _both(ctx, p, plain, opts)
    ctx.set_option("groups_wg", 1)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & (GROUPS | QUERY_WG) and st_h.path_flags & GROUP, f"not handed back ({st_h.path_flags})"
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, opts.max_results, opts.min_score, opts.min_score_pct)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernels)
        assert not st_n.path_flags & (GROUPS | QUERY_WG) and got_n == got, st_n.path_flags
    finally:
        ctx.set_option("groups_wg", -1)
    p = _finish(w, 1)                                          # a fresh snapshot of the same segments
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


# ---- 10. many queries from host memory, and a deadline ------------------------------------------------------------------------------------

def test_a_batch_uploaded_in_pieces_and_a_deadline(tiny):
    """2400 queries of 450 hashes from host memory: more than the chip's 1024 workgroups (every launch hands its queries out through a
    counter of its own) and large enough to be uploaded in pieces -- the groups are walked piece by piece.  == the batch under 0.  With a
    deadline of 1 ms the call is a timeout or complete and right, nothing else; the next call without a deadline is right"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1920)
    w, _, _ = _two_groups(Pair, ctx, rng)
    p = _finish(w, 1)
    queries = _queries(rng, w, 24, qlen=450) * 100
    assert sum(len(q) for q in queries) >= 1 << 20
    ctx.set_option("groups_wg", 0)
    try:
        want, st0 = p.reader.search_batch(queries, fpx.http_options())
        assert not st0.path_flags & GROUPS
        ctx.set_option("groups_wg", 1)
        got, st = p.reader.search_batch(queries, fpx.http_options())
        assert st.path_flags & TAKEN == TAKEN, st.path_flags
        assert got == want and wg.figures(st) == wg.figures(st0), (wg.figures(st), wg.figures(st0))
        try:
            timed, _ = p.reader.search_batch(queries, fpx.http_options(), timeout_ms=1)
            assert timed == want
        except fpx.SearchTimeout as e:
            assert e.status == -2
        again, st2 = p.reader.search_batch(queries, fpx.http_options())
        assert again == want and st2.path_flags & TAKEN == TAKEN, st2.path_flags
    finally:
        ctx.set_option("groups_wg", -1)
