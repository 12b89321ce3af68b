"""k_search_side (csrc/fpx_qside.hpp, option side_wg = 1): the file segments NEXT TO the group of a live index -- checkpoints kept decoded,
a merged segment direct-addressed on its own -- searched a QUERY PER WORKGROUP instead of by the pipeline (keys, radix pass, k_probe_small,
k_probe_direct, partition, k_score).  fpx_stats.path_flags bit 9 (512) says that a batch, or its part 1, ran the kernel.

Every case goes through Pair.check under side_wg = 1 (results and every query's scanned blocks / docs == the oracle's) and is then run
again under side_wg = 0 and compared byte for byte: results, scanned_blocks, scanned_docs, probes, hits, per-query blocks / docs and the
growth of the context's scan histograms (nothing unbucketed).  The shapes are the smallest that reach each branch of the kernel."""
import numpy as np
import pytest

import wg_harness as wg
from wg_harness import QS_MAX_HASHES, QUERY_WG, SECOND_TRIP, SIDE, TWO_PARTS, U64, aimed as _aimed, rand_items as _rand_items

pytestmark = pytest.mark.gpu

HOT, SHARED, CROWD = 0x12345678, 0x0BADF00D, 0x51515151
OPTIONS = ("side_wg", "query_wg", "direct_min_items")


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.fixture
def live(env, monkeypatch):
    """every file segment a direct-addressed candidate unless a test says otherwise, groups packed; the options reset afterwards"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1) as e:
        yield e


class World(wg.World):
    """a Pair filled the way a live index grows: a packed group, checkpoints in blocks (small decoded: what file() takes a segment for
    unless told), merged segments that are direct-addressed alone, memory segments"""

    def __init__(self, Pair, ctx):
        super().__init__(Pair, ctx, packed=1, form="blocks")

    def group(self, rng, cols, per, nh, first=1):
        """`cols` columns with SHARED a list of 2 / 3 / 4 / 70 docs, met in a snapshot: a packed group -> the first free doc.  (In place of
        the harness's columns() + group(): direct_min_items is set once, and every segment there is must be in the group)"""
        self.ctx.set_option("direct_min_items", 0)
        for s in range(cols):
            ids = np.arange(first + s * per, first + (s + 1) * per)
            self.file(_rand_items(rng, ids, nh, [(SHARED, ids[: [2, 3, 4, 70][s % 4]])]), ids, form=None)
        self.p.finish()
        assert all(g.grouped for g in self.p.gpu_segs), [g.layout_reason for g in self.p.gpu_segs]
        return first + cols * per


def _both(ctx, p, queries, opts, want=0, want_not=0):
    """Pair.check under side_wg = 1 with the path bits asserted, then the batch under side_wg = 1 and 0, everything equal"""
    return wg.both(ctx, p, queries, opts, "side_wg", 1, clear=SIDE, want=want, want_not=want_not,
                   compare=wg.FOUR)      # (blocks, docs, probes and hits: this suite never compared algorithmic_bytes)


def _option_sets(fpx):
    return [fpx.http_options(), fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0),
            fpx.SearchOptions(max_results=7, min_score=4, min_score_pct=60)]


def _two_part_world(Pair, ctx, rng):
    """a packed group of 4 columns x 3000 docs x 40 hashes; next to it three checkpoints of 1000 docs x 48 hashes (blocks, decoded small), one
    merged segment of 2500 docs (direct-addressed alone) and three memory segments"""
    w = World(Pair, ctx)
    nxt = w.group(rng, 4, 3000, 40)
    for s in range(3):
        ids = np.arange(nxt, nxt + 1000)
        w.file(_rand_items(rng, ids, 48, [(SHARED, ids[:7]), (HOT, ids[:600])]), ids)
        nxt += 1000
    ids = np.arange(nxt, nxt + 2500)
    w.file(_rand_items(rng, ids, 48, [(SHARED, ids[:70])]), ids, form="alone")
    nxt += 2500
    for m in range(3):
        ids = np.arange(nxt, nxt + 60)
        w.memory(_rand_items(rng, ids, 48, [(SHARED, ids[:3])]), ids)
        nxt += 60
    return w, w.finish()


def test_two_parts_the_side_segments_a_query_per_workgroup(live):
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(808)
    w, p = _two_part_world(Pair, ctx, rng)
    assert not any(g.grouped for g in p.gpu_segs[4:]), [g.layout_reason for g in p.gpu_segs]
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED, SHARED]) for i in range(66)]      # (a query in eleven aims at each addition)
    queries[3] = np.concatenate([queries[3][:990], np.array([HOT], dtype=np.uint32)])
    for opts in _option_sets(fpx):
        got, st = _both(ctx, p, queries, opts, want=SIDE | TWO_PARTS | QUERY_WG)
    found_in = [sum(1 for g in got if g and lo <= g[0][0] <= hi) for lo, hi in ((1, 12000), (12001, 15000), (15001, 17500), (17501, 17680))]
    assert all(n >= 3 for n in found_in), found_in            # the group, the checkpoints, the merged one, the memory segments
    # resident in HBM: the same path, the same answers
    ctx.set_option("side_wg", 1)
    try:
        for opts in _option_sets(fpx):
            want, _ = p.reader.search_batch(queries, opts)
            qb = fpx.QueryBatch(ctx, queries=queries, options=opts)
            o, n, st_r = fpx.search_resident(p.reader, qb)
            qb.release()
            assert st_r.path_flags & (SIDE | TWO_PARTS | QUERY_WG) == SIDE | TWO_PARTS | QUERY_WG, st_r.path_flags
            assert fpx.results_to_lists(o, n) == want
    finally:
        ctx.set_option("side_wg", -1)
    # the option is off by default
    _, st_d = p.reader.search_batch(queries, fpx.http_options())
    assert not st_d.path_flags & SIDE and st_d.path_flags & TWO_PARTS


def test_a_whole_snapshot_of_side_segments_only(live):
    """a young index: two checkpoints and one direct-addressed segment, no group -- not partial: the relative cut-off runs in k_finish"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(809)
    w = World(Pair, ctx)
    nxt = 1
    for s in range(2):
        ids = np.arange(nxt, nxt + 1000)
        w.file(_rand_items(rng, ids, 48, [(SHARED, ids[:5])]), ids)
        nxt += 1000
    ids = np.arange(nxt, nxt + 1500)
    w.file(_rand_items(rng, ids, 48, [(SHARED, ids[:9])]), ids, form="alone")
    p = w.finish()
    assert [bool(g.direct) for g in p.gpu_segs] == [False, False, True] and not any(g.grouped for g in p.gpu_segs)
    queries = [_aimed(rng, w.items[i % 3], [1000, 300, 64, 1500][i % 4], [SHARED]) for i in range(40)]
    for opts in _option_sets(fpx) + [fpx.SearchOptions(max_results=40, min_score=10, min_score_pct=100)]:
        _both(ctx, p, queries, opts, want=SIDE, want_not=TWO_PARTS | QUERY_WG)


def test_the_caps_and_the_list_forms(live):
    """a small segment of 64-byte blocks with a hash of 1500 docs (the walk stops after four blocks), one of 512-byte blocks with a hash of
    3000 (it stops beyond 1000 docs); a direct-addressed segment with lists of 2, 3, 4 and 70 docs (the inline head with T set and clear, a
    list read on by the wave).  One query holds all of them."""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(810)
    w = World(Pair, ctx)
    ids = np.arange(1, 2001)
    w.file(_rand_items(rng, ids, 8, [(HOT, ids[:1500]), (SHARED, ids[:2])]), ids, block_size=64)
    ids = np.arange(2001, 5201)
    w.file(_rand_items(rng, ids, 24, [(HOT + 1, ids[:3000]), (SHARED, ids[:5])]), ids)
    ids = np.arange(5201, 7201)
    lists = [(0x0BADF002, ids[:2]), (0x0BADF003, ids[:3]), (0x0BADF004, ids[:4]), (0x0BADF070, ids[:70]), (HOT, ids[:1200])]
    w.file(_rand_items(rng, ids, 32, lists), ids, form="alone")
    p = w.finish()
    assert [bool(g.direct) for g in p.gpu_segs] == [False, False, True]
    special = [HOT, HOT + 1, SHARED, 0x0BADF002, 0x0BADF003, 0x0BADF004, 0x0BADF070]
    queries = [_aimed(rng, w.items[i % 3], 400, special if i == 0 else special[i % 7: i % 7 + 2]) for i in range(12)]
    for opts in (fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0), fpx.http_options()):
        got, st = _both(ctx, p, queries, opts, want=SIDE)
    want, ost = p.osnap.search(queries[0], 100, 3, 0, with_stats=True)
    assert ost.scanned_docs > 2000, ost.scanned_docs          # (the 3000-doc run and the 1200-doc list were walked past 1000 docs each)


def test_superseded_docs_among_the_side_segments(live):
    """a doc of checkpoint 0 written again in checkpoint 2 with other hashes, one tombstoned in checkpoint 1, a doc of the merged segment
    rewritten in a memory segment: the old versions are counted in scanned_docs and not returned"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(811)
    w = World(Pair, ctx)
    nxt = w.group(rng, 4, 3000, 40)
    c0 = np.arange(nxt, nxt + 1000)
    rewritten, tombstoned = int(c0[17]), int(c0[99])
    w.file(_rand_items(rng, c0, 48), c0)
    nxt += 1000
    ids = np.concatenate([[tombstoned], np.arange(nxt, nxt + 1000)])
    w.file(_rand_items(rng, ids[1:], 48), ids, alive=np.array([0] + [1] * 1000, dtype=np.uint8))
    nxt += 1000
    ids = np.concatenate([[rewritten], np.arange(nxt, nxt + 1000)])
    new_rows = (rng.integers(0, 1 << 32, 48, dtype=U64) << U64(32)) | U64(rewritten)
    w.file(np.unique(np.concatenate([_rand_items(rng, ids[1:], 48), new_rows])), ids)
    nxt += 1000
    merged = np.arange(nxt, nxt + 2500)
    moved = int(merged[5])
    w.file(_rand_items(rng, merged, 48), merged, form="alone")
    nxt += 2500
    ids = np.concatenate([[moved], np.arange(nxt, nxt + 60)])
    moved_rows = (rng.integers(0, 1 << 32, 48, dtype=U64) << U64(32)) | U64(moved)
    w.memory(np.unique(np.concatenate([_rand_items(rng, ids[1:], 48), moved_rows])), ids)
    p = w.finish()

    def rows(items, doc):
        return (items[(items & U64(0xFFFFFFFF)) == U64(doc)] >> U64(32)).astype(np.uint32)

    old = {rewritten: rows(w.items[4], rewritten), tombstoned: rows(w.items[4], tombstoned), moved: rows(w.items[7], moved)}
    new = {rewritten: rows(w.items[6], rewritten), moved: rows(w.items[8], moved)}
    queries = [_aimed(rng, w.items[4 + i % 5], 600) for i in range(20)]
    for i, d in enumerate(old):
        queries[i] = np.concatenate([old[d], rng.integers(0, 1 << 32, 500, dtype=U64).astype(np.uint32)])
    for i, d in enumerate(new):
        queries[4 + i] = np.concatenate([new[d], rng.integers(0, 1 << 32, 500, dtype=U64).astype(np.uint32)])
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    got, st = _both(ctx, p, queries, opts, want=SIDE | TWO_PARTS)
    for i, d in enumerate(old):
        assert all(doc != d for doc, _ in got[i]), (i, d, got[i][:4])
        _, ost = p.osnap.search(queries[i], 100, 3, 0, with_stats=True)
        assert ost.scanned_docs >= 48, ost.scanned_docs         # (the old version's postings were walked)
    assert got[4][0] == (rewritten, 48) and got[5][0] == (moved, 48), (got[4][:2], got[5][:2])
    _both(ctx, p, queries, fpx.http_options(), want=SIDE | TWO_PARTS)


def test_edge_queries(live):
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(812)
    w = World(Pair, ctx)
    ids = np.arange(1, 1001)
    w.file(_rand_items(rng, ids, 48, [(0, ids[:2]), (0xFFFFFFFF, ids[5:8])]), ids)
    ids = np.arange(1001, 2001)
    w.file(_rand_items(rng, ids, 48, lo=0x20000000, hi=0xE0000000), ids)
    ids = np.arange(2001, 4001)
    w.file(_rand_items(rng, ids, 48, lo=0x10000000, hi=0xF0000000), ids, form="alone")
    p = w.finish()
    # hashes absent from the second checkpoint: inside a block (the reference visits one block: a cell of code 1 or an absent hash next
    # to items), in the gap between two blocks where there is one, and outside every block (no visit: code 2) -- by the oracle's count
    seg1 = oracle.Snapshot([p.orc_file[1]], [])
    hs = np.unique((w.items[1] >> U64(32)).astype(np.uint64))
    wide = np.nonzero(np.diff(hs) > (1 << 17))[0][:600]
    visited = {0: [], 1: []}
    for k in wide:
        h = int(hs[k] + (hs[k + 1] - hs[k]) // 2)
        _, ost = seg1.search(np.array([h], dtype=np.uint32), 10, 1, 0, with_stats=True)
        if len(visited[ost.scanned_blocks]) < 3:
            visited[ost.scanned_blocks].append(h)
    assert visited[1], "no absent hash inside a block"
    outside = [0x100, 0x1FFFFFFF, 0xE0000001, 0xFFFFFF00]
    for h in outside:
        assert seg1.search(np.array([h], dtype=np.uint32), 10, 1, 0, with_stats=True)[1].scanned_blocks == 0
    cells = np.array(visited[0] + visited[1] + outside, dtype=np.uint32)
    alone_h = np.unique((w.items[2] >> U64(32)).astype(np.uint32))
    below_above = np.array([int(alone_h[0]) - 1, int(alone_h[0]) - 4096, int(alone_h[-1]) + 1, int(alone_h[-1]) + 4096, int(alone_h[0]), int(alone_h[-1])], dtype=np.uint32)
    own = (w.items[0][(w.items[0] & U64(0xFFFFFFFF)) == U64(300)] >> U64(32)).astype(np.uint32)
    full = np.concatenate([own, rng.integers(0, 1 << 32, QS_MAX_HASHES - len(own), dtype=U64).astype(np.uint32)])
    assert len(full) == QS_MAX_HASHES
    queries = [np.zeros(0, dtype=np.uint32),
               np.full(500, int(own[0]), dtype=np.uint32),
               np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32),
               np.concatenate([below_above, own[:20]]),
               np.concatenate([cells, own[:20]]),
               np.concatenate([cells, below_above, np.array([0, 0xFFFFFFFF], dtype=np.uint32), _aimed(rng, w.items[2], 700)]),
               full,
               _aimed(rng, w.items[1], 1000)]
    opts = fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)
    got, st = _both(ctx, p, queries, opts, want=SIDE)
    assert got[0] == [] and got[1] == [] and got[6][0][0] == 300
    _both(ctx, p, queries, fpx.SearchOptions(max_results=100, min_score=1000, min_score_pct=0), want=SIDE)
    # a query of QS_MAX_HASHES + 1 hashes does not fit the kernel's hash set; a floor of 2 is the pipeline's
    longer = [np.concatenate([full, np.array([12345], dtype=np.uint32)]), queries[7]]
    _both(ctx, p, longer, opts, want_not=SIDE)
    _both(ctx, p, queries, fpx.SearchOptions(max_results=100, min_score=2, min_score_pct=0), want_not=SIDE)


def test_crowded_queries_take_the_shared_list(live):
    """250 docs of a checkpoint share thirty hashes: more candidates than a query's four slots, than the 32 of its LDS buffer and than the
    exact table's 192 (classes) -- the shared list and the second finish (path_flags bit 1)"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(813)
    w = World(Pair, ctx)
    ids = np.arange(1, 1501)
    w.file(_rand_items(rng, ids, 40, [(CROWD + k * 7919, ids[100:350]) for k in range(30)]), ids)
    ids = np.arange(1501, 3001)
    w.file(_rand_items(rng, ids, 40, [(CROWD + k * 7919, ids[:20]) for k in range(30)]), ids, form="alone")
    p = w.finish()
    crowd = np.array([CROWD + k * 7919 for k in range(30)], dtype=np.uint32)
    queries = []
    for i in range(12):
        q = np.concatenate([crowd[: 30 if i % 3 == 0 else 26 + i % 4], rng.integers(0, 1 << 32, 900, dtype=U64).astype(np.uint32)])
        rng.shuffle(q)
        queries.append(q)
    for opts in (fpx.SearchOptions(max_results=100, min_score=25, min_score_pct=0), fpx.SearchOptions(max_results=100, min_score=20, min_score_pct=10)):
        got, st = _both(ctx, p, queries, opts, want=SIDE | SECOND_TRIP)
    assert len(got[0]) == 100


def test_records_beyond_the_lds_array_are_handed_back(live):
    """a query holding twelve hashes of 1000+ docs each across the checkpoints: more records than the 8192 its workgroup keeps.  An ordinary
    fallback: part 1 is redone by the pipeline (bit 9 clear in the final statistics), the answers are the oracle's, and so are the next batch's"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(814)
    w = World(Pair, ctx)
    nxt = w.group(rng, 4, 3000, 40)
    hots = [0x40000000 + 977 * k for k in range(12)]
    for s in range(3):
        ids = np.arange(nxt, nxt + 2000)
        w.file(_rand_items(rng, ids, 24, [(k, ids[:1500]) for k in hots[s::3]]), ids)
        nxt += 2000
    p = w.finish()
    plain = [_aimed(rng, w.items[4 + i % 3], 1000) for i in range(16)]
    heavy = list(plain)
    heavy[5] = np.concatenate([plain[5][:900], np.array(hots, dtype=np.uint32)])
    got, st = _both(ctx, p, plain, fpx.http_options(), want=SIDE | TWO_PARTS)
    ctx.set_option("side_wg", 1)
    try:
        got_h, st_h = p.reader.search_batch(heavy, fpx.http_options())
        assert not st_h.path_flags & SIDE and st_h.path_flags & TWO_PARTS, f"12 x 1000+ records fit 8192? ({st_h.path_flags})"
        _, ost = p.osnap.search(heavy[5], 40, None, 10, with_stats=True)
        assert ost.scanned_docs > 8192, ost.scanned_docs
        for q, g in zip(heavy, got_h):
            assert g == p.osnap.search(q, 40, None, 10)
        got_n, st_n = p.check(plain, fpx.http_options())      # (the next batches: right whichever path they take)
        assert got_n == got
        ctx.set_option("side_wg", 0)
        got_p, st_p = p.reader.search_batch(heavy, fpx.http_options())
        assert got_p == got_h and (st_p.scanned_blocks, st_p.scanned_docs, st_p.probes, st_p.hits) == (st_h.scanned_blocks, st_h.scanned_docs, st_h.probes, st_h.hits)
    finally:
        ctx.set_option("side_wg", -1)


def test_a_second_group_in_part_one_is_not_eligible(live):
    """two merged segments form a group of their own, which goes with part 1: the pipeline's"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(815)
    w = World(Pair, ctx)
    nxt = w.group(rng, 5, 3000, 40)
    for s in range(2):
        ids = np.arange(nxt, nxt + 900)
        w.file(_rand_items(rng, ids, 40, [(SHARED, ids[:11])]), ids, form="alone")
        nxt += 900
    ids = np.arange(nxt, nxt + 500)
    w.file(_rand_items(rng, ids, 40), ids)
    p = w.finish()
    infos = [g.group_info() for g in p.gpu_segs[:7]]
    assert all(i is not None for i in infos) and infos[5]["columns"] == 2, infos
    queries = [_aimed(rng, w.items[i % len(w.items)], 1000, [SHARED]) for i in range(24)]
    _both(ctx, p, queries, fpx.http_options(), want=TWO_PARTS | QUERY_WG, want_not=SIDE)


def test_doc_ids_at_the_top_of_the_range(live):
    """side segments with docs in 0xFFFFFF00 .. 0xFFFFFFFF and across 2^31, next to a group of low ids: records, table keys and candidates
    carry absolute 32-bit ids"""
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(816)
    w = World(Pair, ctx)
    w.group(rng, 4, 3000, 40)
    top = np.arange(0xFFFFFF00, 0x100000000, dtype=np.int64)
    w.file(_rand_items(rng, top, 48, [(SHARED, top[-5:]), (HOT, top[:200])]), top)
    sign = np.arange(0x7FFFFF00, 0x80000100, dtype=np.int64)
    w.file(_rand_items(rng, sign, 48, [(SHARED, sign[250:262]), (HOT, sign[200:300])]), sign, form="alone")
    p = w.finish()
    assert bool(p.gpu_segs[5].direct) and not p.gpu_segs[5].grouped and not p.gpu_segs[4].direct

    def rows(items, doc):
        return (items[(items & U64(0xFFFFFFFF)) == U64(doc)] >> U64(32)).astype(np.uint32)

    aims = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFF00, 0x7FFFFFFF, 0x80000000, 0x80000001, 0x7FFFFF00, 0x800000FF]
    queries = []
    for i in range(24):
        if i < len(aims):
            own = rows(w.items[4 if aims[i] >= 0xFFFFFF00 else 5], aims[i])
            q = np.concatenate([own, np.array([SHARED, HOT], dtype=np.uint32), rng.integers(0, 1 << 32, 400, dtype=U64).astype(np.uint32)])
        else:
            q = _aimed(rng, w.items[i % len(w.items)], 500, [SHARED, HOT])
        queries.append(q)
    for opts in _option_sets(fpx):
        got, st = _both(ctx, p, queries, opts, want=SIDE | TWO_PARTS)
    for i, d in enumerate(aims):
        assert got[i] and got[i][0][0] == d, (hex(d), got[i][:3])


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_live_worlds(live, seed):
    """the worlds of test_gpu_query_wg.test_random_live_worlds_in_two_parts (the same generator, the same seeds) under side_wg = 1.  The path
    is asserted where the world's forms make it certain: a deleted doc of the group means one part and the pipeline; at most one segment
    direct-addressed alone (two would form a group of their own in part 1) means k_search_side"""
    from test_gpu_query_wg import _items, _query
    fpx, oracle, Pair, ctx = live
    rng = np.random.default_rng(9000 + seed)
    p = Pair(ctx)
    allitems, nxt, commit = [], 1, 1
    ncol = int(rng.integers(2, 7))
    for s in range(ncol):
        per = int(rng.integers(800, 3000))
        items = _items(rng, s, per, nxt, 40)
        p.add_file(items, nxt, nxt + per - 1, commit, np.arange(nxt, nxt + per, dtype=np.uint32))
        allitems.append(items)
        nxt += per + int(rng.integers(0, 50)); commit += 1
    p.finish()
    assert all(g.grouped for g in p.gpu_segs)
    group_docs, n_alone = nxt, 0
    for s in range(int(rng.integers(1, 5))):
        alone = bool(rng.integers(0, 3) == 0)
        n_alone += int(alone)
        ctx.set_option("direct_min_items", 0 if alone else 1 << 20)
        per = int(rng.integers(50, 2500))
        docs = np.arange(nxt, nxt + per, dtype=np.uint64)
        ids, alive = list(range(nxt, nxt + per)), [1] * per
        h = rng.integers(0, 1 << 32, (per, int(rng.integers(8, 64))), dtype=np.uint64)
        parts = [((h << np.uint64(32)) | docs[:, None]).ravel(), (np.uint64(SHARED) << np.uint64(32)) | docs[: min(per, 9)]]
        if rng.integers(0, 2):
            parts.append((np.uint64(HOT) << np.uint64(32)) | docs[: min(per, int(rng.integers(100, 1500)))])
        if seed == 3 and s == 0:
            ids.insert(0, 5); alive.insert(0, 0)               # doc 5 of the group deleted here: a tombstone
        items = np.unique(np.concatenate(parts))
        p.add_file(items, min(ids), max(ids), commit, np.array(ids, dtype=np.uint32), np.array(alive, dtype=np.uint8))
        allitems.append(items)
        nxt += per + int(rng.integers(0, 30)); commit += 1
    ctx.set_option("direct_min_items", -1)
    for m in range(int(rng.integers(0, 4))):
        per = int(rng.integers(5, 80))
        docs = np.arange(nxt, nxt + per, dtype=np.uint64)
        h = rng.integers(0, 1 << 32, (per, 32), dtype=np.uint64)
        items = np.unique(((h << np.uint64(32)) | docs[:, None]).ravel())
        p.add_memory(items, nxt, nxt + per - 1, commit, np.arange(nxt, nxt + per, dtype=np.uint32))
        allitems.append(items)
        nxt += per; commit += 1
    p.finish()
    lens = rng.integers(60, 1500, 40)
    queries = [_query(rng, allitems, i, int(lens[i]), special=bool(i % 3 == 0)) for i in range(40)]
    queries[1] = np.concatenate([queries[1], np.array([HOT, SHARED], dtype=np.uint32)])
    for opts in (fpx.http_options(), fpx.SearchOptions(max_results=int(rng.integers(1, 60)), min_score=int(rng.integers(3, 9)), min_score_pct=int(rng.integers(0, 100)))):
        if seed == 3:
            got, st = _both(ctx, p, queries, opts, want_not=SIDE | TWO_PARTS)
        elif n_alone <= 1:
            got, st = _both(ctx, p, queries, opts, want=SIDE | TWO_PARTS)
        else:
            got, st = _both(ctx, p, queries, opts, want=TWO_PARTS)
    assert any(g and g[0][0] >= group_docs for g in got) and any(g and g[0][0] < group_docs for g in got)
