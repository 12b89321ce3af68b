"""k_search_words (csrc/fpx_qwords.hpp, option words_wg = 1 | 2): a snapshot that is ONE group in DIRECTORY + WORDS form -- every group that
is not dense enough to be packed, or whose doc ids span 2^31 or more -- searched a QUERY PER WORKGROUP instead of by the pipeline (keys,
radix pass, k_probe_group, bins, k_score_bin).  fpx_stats.path_flags bit 11 (2048) says that a batch, or its part 0, ran the kernel; bit 8
with it: its filtered form (words_wg = 2: superseded docs, columns outside the snapshot).

Every case goes through Pair.check under the option (results and every query's scanned blocks / docs == the oracle's) and is then run
again under the option and under words_wg = 0 and compared byte for byte: results, scanned_blocks, scanned_docs, probes, hits,
algorithmic_bytes, per-query blocks / docs and the growth of the context's scan histograms (nothing unbucketed).  The groups are tiny
(group_packed = 0, FPX_DIRECT_MIN_ITEMS = 0): each case is the smallest shape that reaches a branch of the kernel."""
import functools

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import (FILTERED, GROUP, QS_MAX_HASHES, QUERY_WG, SECOND_TRIP, SIDE, TWO_PARTS, U64, WORDS, WORDS_LO as LO, WORDS_HI as HI,
                        aimed as _aimed, figures as _figures, rows as _rows)

pytestmark = pytest.mark.gpu

SHARED, DOUBLE, BIG, HOT, CROWD, LINE = 0x2BADF00D, 0x37770000, 0x42345678, 0x4BCDEF01, 0x51515151, 0x5A5A5A00
OPTIONS = ("words_wg", "side_wg", "query_wg", "direct_min_items")
_usual = wg.usual(SHARED, DOUBLE)
_reset = functools.partial(wg.reset, options=OPTIONS)
_rand_items = functools.partial(wg.rand_items, lo=LO, hi=HI)      # (the columns' random hashes are in [LO, HI) unless a test says otherwise)


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    _reset(e[3])


@pytest.fixture
def tiny(env, monkeypatch):
    """every file segment a direct-addressed candidate unless a test says otherwise, groups in directory + words form"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=0) as e:
        yield e


def World(Pair, ctx):
    """a Pair whose file segments meet in ONE group in directory + words form; checkpoints, a merged segment and memory segments next to it"""
    return wg.World(Pair, ctx, packed=0, lo=LO, hi=HI)


def _both(ctx, p, queries, opts, level=1, want=WORDS | GROUP, want_not=QUERY_WG, also=()):
    """Pair.check under words_wg = level with the path bits asserted, then the batch under the option and under 0, everything equal"""
    return wg.both(ctx, p, queries, opts, "words_wg", level, clear=WORDS, want=want, want_not=want_not, also=also,
                   compare=wg.WITH_BYTES)      # (algorithmic_bytes too)


def _option_sets(fpx):
    return [fpx.http_options(), fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0),
            fpx.SearchOptions(max_results=1, min_score=4, min_score_pct=100)]


def _gap_hashes(oracle, w, col, n=3):
    """hashes of column `col` in gap positions: right behind a block's last hash, no block visited (by the oracle's count)"""
    seg = oracle.Snapshot([w.p.orc_file[col]], [])
    out = []
    for b in range(len(w.index[col]) - 1):
        h = int(w.index[col][b]) + 1
        _, ost = seg.search(np.array([h], dtype=np.uint32), 10, 1, 0, with_stats=True)
        if ost.scanned_blocks == 0 and ost.scanned_docs == 0:
            out.append(h)
        if len(out) == n:
            break
    assert out, "no gap position"
    return out


# ---- 1. both line widths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,block_size", [(5, 512), (9, 512), (5, 64)])
def test_both_line_widths(tiny, cols, block_size):
    """5 columns (lines of 8) and 9 (lines of 16): docs, a double in every column, lists of 2 / 3 / 4 / 70 docs (the inline head with T set and
    clear, a list read on by the wave), a hash of 1100 docs (the cap beyond 1000), noise absent in range, out of every column's range and
    in gap positions; blocks of 64 bytes: the four-block cap with a few dozen docs"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1300 + cols + block_size)
    w = World(Pair, ctx)
    # (blocks of 64 bytes hold a dozen items: a gap position between every two of them costs the direct-addressed form a word, so that
    # case keeps its hashes -- the special ones too -- within 2^27 values)
    lo, hi = (LO, HI) if block_size == 512 else (0x30000000, 0x38000000)
    shared, double, big = (SHARED, DOUBLE, BIG) if block_size == 512 else (0x31ADF00D, 0x33770000, 0x35345678)
    usual = lambda s, ids: [(shared, ids[: [2, 3, 4, 70][s % 4]]), (double, ids[:2])] + ([(big, ids[:1100])] if s == 1 else [])
    p, _ = w.columns(rng, cols, 1500, 64, usual, block_size=block_size, lo=lo, hi=hi)
    gaps = _gap_hashes(oracle, w, 0) + _gap_hashes(oracle, w, cols - 1)
    special = [shared, double, big] + gaps + [1, lo - 1, hi + 5, 0xFFFFFFF0]
    queries = [_aimed(rng, w.items[i % cols], 1000, special if i % 4 == 0 else special[i % 5: i % 5 + 3], lo, hi) for i in range(24)]
    for opts in _option_sets(fpx):
        got, st = _both(ctx, p, queries, opts)
    _, ost = p.osnap.search(queries[0], 100, 3, 0, with_stats=True)
    if block_size == 512:
        assert ost.scanned_docs > 1000 + 70, ost.scanned_docs      # (the hash of 1100 docs was walked past 1000)
    else:
        assert ost.scanned_blocks > 4 * 2 and ost.scanned_docs < 1100, (ost.scanned_blocks, ost.scanned_docs)      # (... stopped after four blocks)
    # the option is off by default
    _, st_d = p.reader.search_batch(queries, fpx.http_options())
    assert not st_d.path_flags & WORDS and st_d.path_flags & GROUP, st_d.path_flags


# ---- 2. wide hashes -------------------------------------------------------------------------------------------------------------

def test_wide_hashes(tiny):
    """16 columns: a hash that is a double in all of them (32 words: twenty beyond the lane's twelve) and one that is a list in all of
    them (sixteen lists for one hash, some longer than their head)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1320)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 16, 600, 64, lambda s, ids: [(DOUBLE, ids[:2]), (SHARED, ids[: [3, 5, 70, 4, 130, 6][s % 6]])])
    queries = [_aimed(rng, w.items[i % 16], 600, [DOUBLE, SHARED][: 1 + i % 2] if i % 3 else [SHARED, DOUBLE]) for i in range(24)]
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts)
    want, ost = p.osnap.search(queries[0], 100, 3, 0, with_stats=True)
    assert ost.scanned_docs >= 32 + 16 * 3, ost.scanned_docs


# ---- 3. crowded directory lines -------------------------------------------------------------------------------------------------

def _line_queries(rng, w, cols):
    line = np.arange(LINE, LINE + 32, dtype=np.uint32)
    qs = [np.concatenate([line, _aimed(rng, w.items[i % cols], 300)]) for i in range(6)]
    qs += [np.concatenate([line[i::5], _aimed(rng, w.items[i % cols], 300)]) for i in range(10)]
    qs += [np.concatenate([line[i: i + 1], rng.integers(0, 1 << 32, 40, dtype=U64).astype(np.uint32)]) for i in range(0, 32, 3)]
    return qs


@pytest.mark.parametrize("cols,have", [(8, 8), (16, 13)])
def test_a_line_with_more_positions_than_double_bits(tiny, cols, have):
    """32 consecutive hash values in every column of an 8-column group (256 positions, 128 double bits) and in 13 columns of a 16-column
    one (416, 384 bits): a line with more positions than bits has none set"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1330 + cols)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, cols, 500, 48, lambda s, ids: [(LINE + i, ids[i: i + 1 + (i % 7 == 0)]) for i in range(32)] if s < have else [])
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    got, st = _both(ctx, p, _line_queries(rng, w, cols), opts)
    assert got[0] and got[0][0][1] >= 3


def test_doubles_across_the_double_words(tiny):
    """the same 32 hash values in 3 columns of an 8-column group -- 96 positions --, with hashes of exactly two docs at positions below 32,
    between 32 and 64 and above 64, one of them at bit 31 of the line: the mask of a hash's doubles straddles two double words"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1333)
    w = World(Pair, ctx)
    in_cols = (1, 4, 6)
    # position of (hash i, the k-th of the three columns) = 3 i + k: 31 = (10, 1); 4 = (1, 1); 40 = (13, 1); 70 = (23, 1); 33 = (11, 0)
    two = {(1, 4), (10, 4), (13, 4), (23, 4), (11, 1), (10, 6), (31, 6)}
    p, _ = w.columns(rng, 8, 500, 48, lambda s, ids: [(LINE + i, ids[i: i + 1 + ((i, s) in two)]) for i in range(32)] if s in in_cols else [])
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    queries = _line_queries(rng, w, 8)
    got, st = _both(ctx, p, queries, opts)
    _, ost = p.osnap.search(queries[0], 100, 3, 0, with_stats=True)
    assert ost.scanned_docs >= 96 + len(two), ost.scanned_docs


# ---- 4. query shapes ------------------------------------------------------------------------------------------------------------

@pytest.fixture
def shapes(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1340)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 5, 1500, 64, lambda s, ids: _usual(s, ids) + [(0, ids[:2]), (0xFFFFFFFF, ids[5:8])][: 2 if s % 2 == 0 else 0], lo=0, hi=1 << 32)
    return fpx, ctx, rng, w, p


def test_query_shapes(shapes):
    """lengths 0, 1, 256, 257 and 4096, duplicates inside a query, the hashes 0 and 0xFFFFFFFF once and twice; max_results 1 and 100,
    min_score_pct 0 and 100"""
    fpx, ctx, rng, w, p = shapes
    own = _rows(w.items[0], 300)
    full = np.concatenate([own, rng.integers(0, 1 << 32, QS_MAX_HASHES - len(own), dtype=U64).astype(np.uint32)])
    queries = [np.zeros(0, dtype=np.uint32),
               own[:1],
               np.concatenate([own, rng.integers(0, 1 << 32, 256 - len(own), dtype=U64).astype(np.uint32)]),
               np.concatenate([own, rng.integers(0, 1 << 32, 257 - len(own), dtype=U64).astype(np.uint32)]),
               full,
               np.full(500, int(own[0]), dtype=np.uint32),
               np.concatenate([own, own, own[:7], np.array([SHARED, SHARED, DOUBLE], dtype=np.uint32)]),
               np.array([0, 0xFFFFFFFF, 5, 6, 7], dtype=np.uint32),
               np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32),
               _aimed(rng, w.items[3], 1000, [0, 0xFFFFFFFF, SHARED])]
    for opts in (fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0), fpx.SearchOptions(max_results=1, min_score=3, min_score_pct=100),
                 fpx.SearchOptions(max_results=100, min_score=1000, min_score_pct=0)):
        got, st = _both(ctx, p, queries, opts)
    assert got[0] == [] and got[1] == []
    got, _ = _both(ctx, p, queries, fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0))
    assert got[2][0][0] == 300 and got[3][0][0] == 300 and got[4][0][0] == 300 and got[6][0] == (300, len(own))
    # a batch of one (the single query's own path, whatever the option says)
    _both(ctx, p, queries[4:5], fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0), want=0, want_not=0)


def test_more_queries_than_workgroups(shapes):
    """2100 queries of 8 hashes: more than the 1024 workgroups an MI355X holds -- workgroups take a second and a third query, and what
    a query left in LDS must not reach the next"""
    fpx, ctx, rng, w, p = shapes
    queries = []
    for i in range(2100):
        doc = 1 + (i * 37) % 7500
        q = np.concatenate([_rows(w.items[(doc - 1) // 1500], doc)[: 3 + i % 5], np.array([SHARED, 0][: i % 3], dtype=np.uint32)])
        queries.append(np.concatenate([q, rng.integers(0, 1 << 32, 8 - len(q), dtype=U64).astype(np.uint32)]) if len(q) < 8 else q[:8])
    got, st = _both(ctx, p, queries, fpx.SearchOptions(max_results=10, min_score=3, min_score_pct=0))
    assert sum(1 for g in got if g) > 1500


# ---- 5. not taken ---------------------------------------------------------------------------------------------------------------

def test_batches_and_groups_the_kernel_does_not_take(shapes):
    fpx, ctx, rng, w, p = shapes
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    plain = [_aimed(rng, w.items[i % 5], 600, [SHARED]) for i in range(8)]
    longer = plain[:3] + [np.concatenate([rng.integers(0, 1 << 32, QS_MAX_HASHES, dtype=U64).astype(np.uint32), _rows(w.items[0], 9)[:1]])]
    assert len(longer[3]) == QS_MAX_HASHES + 1
    _both(ctx, p, longer, opts, want=GROUP, want_not=WORDS)
    _both(ctx, p, plain, fpx.SearchOptions(max_results=100, min_score=2, min_score_pct=0), want=GROUP, want_not=WORDS)
    _both(ctx, p, plain, opts)                                # (the same batch, a floor of 3: taken)


def test_a_packed_group_is_k_search_querys(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    _reset(ctx)
    ctx.set_option("group_packed", 1)
    try:
        rng = np.random.default_rng(1351)
        w = World(Pair, ctx)
        for s in range(3):
            ids = np.arange(1 + s * 1500, 1 + (s + 1) * 1500)
            w.file(_rand_items(rng, ids, 64, _usual(s, ids)), ids)
        p = w.finish()
        assert p.gpu_segs[0].group_info()["packed"] == 1
        queries = [_aimed(rng, w.items[i % 3], 600, [SHARED]) for i in range(8)]
        _both(ctx, p, queries, fpx.http_options(), want=QUERY_WG, want_not=WORDS)
    finally:
        _reset(ctx)


def _reinserting_world(Pair, ctx, rng, cols=5, per=1500):
    """the newest column writes again, with their SAME hashes, a plain doc of column 0, a doc in column 2's list of four SHARED docs and one
    in column 3's list of 70"""
    w = World(Pair, ctx)
    again = [17, 2 * per + 2, 3 * per + 5]
    for s in range(cols):
        ids = list(range(1 + s * per, 1 + (s + 1) * per))
        items = _rand_items(rng, ids, 64, _usual(s, np.array(ids)))
        if s == cols - 1:
            for d in again:
                src = w.items[(d - 1) // per]
                items = np.unique(np.concatenate([items, src[(src & U64(0xFFFFFFFF)) == U64(d)]]))
                ids.append(d)
        w.file(items, sorted(ids))
    return w, w.group(cols), again


def test_a_filtered_group_under_1_is_the_pipelines(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1352)
    w, p, again = _reinserting_world(Pair, ctx, rng)
    queries = [_aimed(rng, w.items[i % 5], 600, [SHARED]) for i in range(8)]
    _both(ctx, p, queries, fpx.http_options(), level=1, want=GROUP, want_not=WORDS | FILTERED)


# ---- 6. crowded candidates ------------------------------------------------------------------------------------------------------

def test_crowded_queries_take_the_shared_list(tiny):
    """200 docs of a column share thirty hashes: more candidates than a query's four slots, than the 32 of its LDS buffer and than the
    exact table's 192 (classes) -- the shared list and the second finish (path_flags bit 1)"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1360)
    w = World(Pair, ctx)
    crowd = np.array([CROWD + k * 7919 for k in range(30)], dtype=np.uint32)
    p, _ = w.columns(rng, 4, 1200, 40, lambda s, ids: [(int(c), ids[100:300] if s == 0 else ids[:20]) for c in crowd] if s < 2 else [])
    queries = []
    for i in range(12):
        q = np.concatenate([crowd[: 30 if i % 3 == 0 else 26 + i % 4], rng.integers(0, 1 << 32, 900, dtype=U64).astype(np.uint32)])
        rng.shuffle(q)
        queries.append(q)
    for opts in (fpx.SearchOptions(max_results=100, min_score=25, min_score_pct=0), fpx.SearchOptions(max_results=100, min_score=20, min_score_pct=10)):
        got, st = _both(ctx, p, queries, opts, want=WORDS | GROUP | SECOND_TRIP)
    assert len(got[0]) == 100


# ---- 7. hand-back ---------------------------------------------------------------------------------------------------------------

def test_records_beyond_the_lds_array_are_handed_back(tiny):
    """one hash with 1000 docs in each of 9 columns: 9000 records, the array takes 8192.  The batch is the pipeline's (bit 11 clear), so is
    the next one on that snapshot (the back-off); a fresh snapshot takes the kernel again"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1370)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 9, 1200, 24, lambda s, ids: [(HOT, ids[:1000])])
    plain = [_aimed(rng, w.items[i % 9], 600) for i in range(12)]
    plain = [q[q != HOT] for q in plain]                       # (five docs in six hold HOT themselves)
    heavy = list(plain)
    heavy[5] = np.concatenate([plain[5][:500], np.array([HOT], dtype=np.uint32)])
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    got, st = _both(ctx, p, plain, opts)
    ctx.set_option("words_wg", 1)
    try:
        got_h, st_h = p.reader.search_batch(heavy, opts)
        assert not st_h.path_flags & WORDS and st_h.path_flags & GROUP, f"9 x 1000 records fit 8192? ({st_h.path_flags})"
        _, ost = p.osnap.search(heavy[5], 100, 3, 0, with_stats=True)
        assert ost.scanned_docs > 8192, ost.scanned_docs
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, 100, 3, 0)
        got_n, st_n = p.reader.search_batch(plain, opts)       # (the next batch of that snapshot stays off the kernel)
        assert not st_n.path_flags & WORDS and got_n == got, st_n.path_flags
        ctx.set_option("words_wg", 0)
        got_p, st_p = p.reader.search_batch(heavy, opts)
        assert got_p == got_h and _figures(st_p) == _figures(st_h)
    finally:
        ctx.set_option("words_wg", -1)
    p.finish()                                                 # a fresh snapshot of the same segments
    got_f, _ = _both(ctx, p, plain, opts)
    assert got_f == got


# ---- 8. memory segments ---------------------------------------------------------------------------------------------------------

def _memory_segments(w, rng, nxt, n, extra=lambda m, ids: []):
    for m in range(n):
        ids = np.arange(nxt, nxt + 60)
        w.memory(_rand_items(rng, ids, 64, [(SHARED, ids[:3])] + extra(m, ids)), ids)
        nxt += 60
    return nxt


def test_memory_segments_next_to_the_group(tiny):
    """four memory segments with docs of their own and hashes shared with the group's docs: the MEM instantiation"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1380)
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 5, 1500, 64, _usual)
    shared_rows = _rows(w.items[1], 1501 + 40)[:30]
    _memory_segments(w, rng, nxt, 4, lambda m, ids: [(int(h), ids[10:11]) for h in shared_rows] if m == 2 else [])
    p = w.finish()
    assert p.reader.snapshot.info()["memory"] == 4
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(27)]
    queries[0] = np.concatenate([_rows(w.items[1], 1501 + 40), rng.integers(0, 1 << 32, 400, dtype=U64).astype(np.uint32)])
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts)
    assert sum(1 for g in got if g and g[0][0] >= nxt) >= 3     # found in the memory segments
    assert {d for d, _ in got[0]} >= {1501 + 40, nxt + 2 * 60 + 10}, got[0][:4]


# ---- 9. the filtered form -------------------------------------------------------------------------------------------------------

def test_filtered_reinsert_with_the_same_hashes_inside_the_group(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1390)
    w, p, again = _reinserting_world(Pair, ctx, rng, cols=9, per=1000)
    queries = [_aimed(rng, w.items[i % 9], 800, [SHARED, DOUBLE]) for i in range(24)]
    for i, d in enumerate(again):
        queries[i] = np.concatenate([_rows(w.items[(d - 1) // 1000], d), np.array([SHARED], dtype=np.uint32), rng.integers(0, 1 << 32, 500, dtype=U64).astype(np.uint32)])
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts, level=2, want=WORDS | GROUP | FILTERED)
    for i, d in enumerate(again):
        assert got[i] and got[i][0][0] == d and [r[0] for r in got[i]].count(d) == 1, (d, got[i][:4])


def test_filtered_reinsert_with_new_hashes_in_a_memory_segment(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1391)
    w = World(Pair, ctx)
    per = 1500
    _, nxt = w.columns(rng, 4, per, 64, _usual)
    gone = [17, 2 * per + 3, 3 * per + 40]                       # (a plain doc, one in a list of 4, one in a list of 70)
    for m in range(3):
        ids = list(range(nxt, nxt + 50))
        items = [_rand_items(rng, ids, 64)]
        if m == 1:
            for d in gone:                                       # written again, with other hashes
                items.append(_rand_items(rng, [d], 64))
                ids.append(d)
        w.memory(np.unique(np.concatenate(items)), sorted(ids))
        nxt += 50
    p = w.finish()
    queries = [_aimed(rng, w.items[i % len(w.items)], 800, [SHARED]) for i in range(24)]
    for i, d in enumerate(gone):                                 # the OLD hashes of the re-inserted docs
        queries[i] = np.concatenate([_rows(w.items[(d - 1) // per], d), np.array([SHARED], dtype=np.uint32), rng.integers(0, 1 << 32, 500, dtype=U64).astype(np.uint32)])
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts, level=2, want=WORDS | GROUP | FILTERED)
    assert all(d not in [r[0] for r in got[i]] for i, d in enumerate(gone)), "a superseded doc was returned"


def test_filtered_tombstones_in_a_memory_segment(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1392)
    w = World(Pair, ctx)
    per = 1500
    _, nxt = w.columns(rng, 4, per, 64, _usual)
    gone = [5, per + 1, 3 * per + 7]                             # (per + 1: one of column 1's three SHARED docs and a DOUBLE doc)
    w.p.add_memory_changes([("delete", d) for d in gone] + [("insert", nxt, rng.integers(LO, HI, 64).tolist())], w.commit)
    p = w.finish()
    queries = [_aimed(rng, w.items[i % 4], 800, [SHARED, DOUBLE]) for i in range(24)]
    for i, d in enumerate(gone):
        queries[i] = np.concatenate([_rows(w.items[(d - 1) // per], d), np.array([SHARED, DOUBLE], dtype=np.uint32), rng.integers(0, 1 << 32, 500, dtype=U64).astype(np.uint32)])
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts, level=2, want=WORDS | GROUP | FILTERED)
    assert not any(r[0] in gone for g in got for r in g), "a deleted doc was returned"


def test_filtered_columns_outside_the_snapshot(tiny):
    """a snapshot of the two newest of a group's four columns: the other two give nothing -- no record, no statistic"""
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1393)
    w = World(Pair, ctx)
    p, _ = w.columns(rng, 4, 1500, 64, _usual)
    q = Pair(ctx)
    q.gpu_segs, q.orc_file = p.gpu_segs[2:], p.orc_file[2:]
    q.finish()
    info = q.reader.snapshot.info()
    assert info["groups"] == 1 and info["direct_solo"] == 0, info
    queries = [_aimed(rng, w.items[i % 4], 800, [SHARED, DOUBLE]) for i in range(24)]      # (half of them aim at docs of the columns left out)
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, q, queries, opts, level=2, want=WORDS | GROUP | FILTERED)
    assert st.probes == 2 * sum(len(np.unique(x)) for x in queries), (st.probes, sum(len(np.unique(x)) for x in queries))
    assert not any(r[0] <= 3000 for g in got for r in g)
    _both(ctx, q, queries, fpx.http_options(), level=1, want=GROUP, want_not=WORDS | FILTERED)


# ---- 10. doc ids ----------------------------------------------------------------------------------------------------------------

def test_doc_ids_up_to_the_top_and_a_wide_span(env, monkeypatch):
    """columns at 1 .., across 2^31 and up to 0xFFFFFFFF: the span keeps the group in directory + words form even with group_packed 1;
    records, table keys and candidates carry absolute 32-bit ids"""
    fpx, oracle, Pair, ctx = env
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    _reset(ctx)
    ctx.set_option("group_packed", 1)
    try:
        rng = np.random.default_rng(1400)
        w = World(Pair, ctx)
        firsts = [1, 0x7FFFFC00, 0xFFFFF800]
        for s, f in enumerate(firsts):
            ids = np.arange(f, f + 2048, dtype=np.int64)
            w.file(_rand_items(rng, ids, 64, [(SHARED, ids[-[2, 3, 70][s]:]), (DOUBLE, ids[-2:]), (HOT, ids[1000:1040])]), ids)
        p = w.group(3)
        aims = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFF800, 0x7FFFFFFF, 0x80000000, 0x80000001, 1, 2048]
        queries = []
        for i in range(24):
            if i < len(aims):
                own = _rows(w.items[2 if aims[i] >= 0xFFFFF800 else 1 if aims[i] > 2048 else 0], aims[i])
                assert len(own) >= 64
                queries.append(np.concatenate([own, np.array([SHARED, DOUBLE, HOT], dtype=np.uint32), rng.integers(0, 1 << 32, 400, dtype=U64).astype(np.uint32)]))
            else:
                queries.append(_aimed(rng, w.items[i % 3], 500, [SHARED, HOT]))
        for opts in _option_sets(fpx)[:2]:
            got, st = _both(ctx, p, queries, opts)
        for i, d in enumerate(aims):
            assert got[i] and got[i][0][0] == d, (hex(d), got[i][:3])
    finally:
        _reset(ctx)


# ---- 11. two parts --------------------------------------------------------------------------------------------------------------

def _live_world(Pair, ctx, rng, level):
    """a group of 5 columns; next to it two checkpoints in blocks (small decoded), one merged segment direct-addressed alone and two memory
    segments; the snapshot made under words_wg = level"""
    w = World(Pair, ctx)
    _, nxt = w.columns(rng, 5, 1500, 64, _usual)
    for s in range(2):
        ids = np.arange(nxt, nxt + 800)
        w.file(_rand_items(rng, ids, 64, [(SHARED, ids[:7])]), ids, form="blocks")
        nxt += 800
    ids = np.arange(nxt, nxt + 2000)
    w.file(_rand_items(rng, ids, 64, [(SHARED, ids[:70])]), ids, form="alone")
    nxt += 2000
    nxt = _memory_segments(w, rng, nxt, 2)
    ctx.set_option("words_wg", level)                         # (the value in force when the snapshot is made)
    try:
        p = w.finish()
    finally:
        ctx.set_option("words_wg", -1)
    assert not any(g.grouped for g in p.gpu_segs[5:8]) and bool(p.gpu_segs[7].direct) and not p.gpu_segs[5].direct, [g.layout_reason for g in p.gpu_segs]
    return w, p, nxt


def test_two_parts_with_a_words_form_part_0(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1410)
    w, p, nxt = _live_world(Pair, ctx, rng, 1)
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(40)]      # (a query in ten aims at each addition)
    for opts in _option_sets(fpx)[:2]:
        got, st = _both(ctx, p, queries, opts, want=WORDS | GROUP | TWO_PARTS, want_not=QUERY_WG | SIDE)
    found_in = [sum(1 for g in got if g and lo <= g[0][0] < hi) for lo, hi in ((1, 7501), (7501, 9101), (9101, 11101), (11101, nxt))]
    assert all(n >= 3 for n in found_in), found_in            # the group, the checkpoints, the merged one, the memory segments
    _both(ctx, p, queries, fpx.http_options(), want=WORDS | GROUP | TWO_PARTS | SIDE, want_not=QUERY_WG, also=(("side_wg", 1),))
    # resident in HBM: the same path, the same answers
    ctx.set_option("words_wg", 1)
    try:
        want, _ = p.reader.search_batch(queries, fpx.http_options())
        qb = fpx.QueryBatch(ctx, queries=queries, options=fpx.http_options())
        o, n, st_r = fpx.search_resident(p.reader, qb)
        qb.release()
        assert st_r.path_flags & (WORDS | TWO_PARTS) == WORDS | TWO_PARTS, st_r.path_flags
        assert fpx.results_to_lists(o, n) == want
    finally:
        ctx.set_option("words_wg", -1)


def test_a_snapshot_made_under_0_is_searched_as_before(tiny):
    fpx, oracle, Pair, ctx = tiny
    rng = np.random.default_rng(1411)
    w, p, nxt = _live_world(Pair, ctx, rng, 0)
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, DOUBLE]) for i in range(20)]
    _both(ctx, p, queries, fpx.http_options(), want=GROUP, want_not=WORDS | TWO_PARTS | QUERY_WG)


# ---- 12. cancellation -----------------------------------------------------------------------------------------------------------

def test_a_deadline_that_has_passed_is_a_timeout_under_both(shapes):
    """25 200 queries of 1000 hashes from host memory against a deadline of 1 ms: the 100 MB of hashes alone need longer than that on the
    link, so the deadline HAS passed when the call first waits -- error.SearchTimeout with the same status under words_wg 1 and 0, no
    results, and the same call without a deadline afterwards is complete and correct"""
    fpx, ctx, rng, w, p = shapes
    distinct = [_aimed(rng, w.items[i % 5], 1000, [SHARED]) for i in range(600)]
    queries = distinct * 42
    status = {}
    try:
        for level in (1, 0):
            ctx.set_option("words_wg", level)
            want, st = p.reader.search_batch(queries, fpx.http_options())
            assert bool(st.path_flags & WORDS) == bool(level), st.path_flags
            with pytest.raises(fpx.SearchTimeout) as e:
                p.reader.search_batch(queries, fpx.http_options(), timeout_ms=1)
            status[level] = e.value.status
            again, st2 = p.reader.search_batch(queries, fpx.http_options())
            assert again == want and bool(st2.path_flags & WORDS) == bool(level)
            assert want[600:1200] == want[:600]
    finally:
        ctx.set_option("words_wg", -1)
    assert status[1] == status[0] == -2, status
    for i in (0, 1, 15, 599):
        assert want[i] == p.osnap.search(queries[i], 40, None, 10), i
