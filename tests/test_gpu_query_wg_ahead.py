"""k_search_query (csrc/fpx_qsearch.hpp) asks for what a query needs BEFORE the query starts: its hashes -- four rounds of them, in registers,
under the tasks and the counting of the query before it --, its offsets (a query earlier still, as soon as the launch's counter has named
it), its floor, the cancel flag, and the offset of an overflowing line's rest next to the line's words.  What was fetched ahead belongs to
ONE query: these tests give a workgroup a second and a third query (the other tests' batches are smaller than the grid of four workgroups
per CU), of lengths that differ from one to the next and sit on the edges of the hash registers (256 a round, 512 a pair, 1024 the four
rounds held, beyond that a rolling window), and put duplicates and overflowing lines on both sides of those edges.  Every case goes through
Pair.check against the oracle -- results and every query's scanned blocks / docs -- and asserts path_flags & 64 (a query per workgroup);
Pair.check's third search asks for per-query statistics: the kernel's QS instantiations."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHARED = 0x0BADF00D
EDGES = [0, 1, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1537, 2049, 4095, 4096]
BASE, POOL = 0x20000000, 6


@pytest.fixture(scope="module")
def env():
    from fpx_testlib import fpx, oracle, Pair
    ctx = fpx.Context(0)
    yield fpx, oracle, Pair, ctx
    ctx.set_option("query_wg", -1)
    ctx.set_option("group_packed", -2)


def _grid():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _opts(fpx):
    return fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=10)


def _col(rng, s, per, first):
    docs = np.arange(first, first + per, dtype=np.uint64)
    h = rng.integers(0, 1 << 32, (per, 48), dtype=np.uint64)
    parts = [((h << np.uint64(32)) | docs[:, None]).ravel(), (np.uint64(SHARED) << np.uint64(32)) | docs[: [2, 3, 4, 70, 5, 2][s % 6]]]
    if s == 0:
        parts.append((np.uint64(0xFFFFFFFF) << np.uint64(32)) | docs[5:8])
    return np.unique(np.concatenate(parts))


def _world(fpx, Pair, ctx, monkeypatch, nseg, per=2500, seed=1109, memory=0):
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("group_packed", 1)
    try:
        rng = np.random.default_rng(seed + nseg)
        p = Pair(ctx)
        allitems = []
        for s in range(nseg):
            first = s * per + 1
            items = _col(rng, s, per, first)
            p.add_file(items, first, first + per - 1, s + 1, np.arange(first, first + per, dtype=np.uint32))
            allitems.append(items)
        for m in range(memory):                                   # fresh writes next to the group: the MEM instantiations
            first = nseg * per + 1 + m * 60
            docs = np.arange(first, first + 60, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (60, 48), dtype=np.uint64)
            items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel(), (np.uint64(SHARED) << np.uint64(32)) | docs[:3]]))
            p.add_memory(items, first, first + 59, nseg + 1 + m, np.arange(first, first + 60, dtype=np.uint32))
            allitems.append(items)
        p.finish()
    finally:
        ctx.set_option("group_packed", -2)
    assert all(g.direct and g.grouped for g in p.gpu_segs[:nseg]), [g.layout_reason for g in p.gpu_segs]
    return p, allitems, rng


def _query(rng, allitems, i, qlen):
    """qlen hashes: up to 24 of a doc's own (it reaches a floor of 3), noise, and in the longer ones SHARED twice and hashes next to the doc's"""
    if qlen == 0:
        return np.zeros(0, dtype=np.uint32)
    src = allitems[i % len(allitems)]
    doc = src[rng.integers(0, len(src))] & np.uint64(0xFFFFFFFF)
    own = (src[(src & np.uint64(0xFFFFFFFF)) == doc] >> np.uint64(32)).astype(np.uint32)[:max(1, min(24, qlen - qlen // 4))]
    parts = [own]
    if qlen >= 64:
        parts.append(np.array([SHARED, 0, 0xFFFFFFFF, SHARED], dtype=np.uint32))
        parts.append((own[:6].astype(np.int64) + rng.integers(-3, 4, min(6, len(own)))).clip(0, 0xFFFFFFFF).astype(np.uint32))
    have = sum(len(x) for x in parts)
    if qlen > have:
        parts.append(rng.integers(0, 1 << 32, qlen - have, dtype=np.uint64).astype(np.uint32))
    q = np.concatenate(parts)[:qlen]
    rng.shuffle(q)
    return q


def _mixed_lengths(rng, B, grid):
    """3 - 40 hashes, the edge lengths as a workgroup's first query (a short one behind it), as its second (a short one before it), two
    different edges in a row, as a query the counter hands out, and as the batch's last"""
    lens = rng.integers(3, 41, B)
    for j, L in enumerate(EDGES):
        a, b, c = 7 * j + 1, 7 * j + 3, 7 * j + 5
        assert c < grid
        lens[a] = L                                               # first; short after long
        if b + grid < B:
            lens[b + grid] = L                                    # second; long after short
        lens[c] = L
        if c + grid < B:
            lens[c + grid] = EDGES[(j + 7) % len(EDGES)]          # two edges in a row
        if 2 * grid + 3 + 7 * j < B:
            lens[2 * grid + 3 + 7 * j] = L                        # handed out by the counter (static assignment: a third query)
    return lens


@pytest.fixture(scope="module")
def big(env):
    """the world of the batches below, B = 3 x grid + 5 queries and what Pair.check said about them (shared: the oracle runs once)"""
    fpx, oracle, Pair, ctx = env
    mp = pytest.MonkeyPatch()
    try:
        p, allitems, rng = _world(fpx, Pair, ctx, mp, 4)
    finally:
        mp.undo()
    grid = _grid()
    B = 3 * grid + 5
    lens = _mixed_lengths(rng, B, grid)
    lens[B - 1] = 769
    queries = [_query(rng, allitems, i, int(n)) for i, n in enumerate(lens)]
    got, st = p.check(queries, _opts(fpx))
    return p, allitems, rng, grid, queries, got, st


def test_first_second_and_later_queries_of_a_workgroup(env, big):
    fpx, oracle, Pair, ctx = env
    p, allitems, rng, grid, queries, got, st = big
    assert st.path_flags & 64, f"the batch did not run k_search_query ({st.path_flags})"
    assert sum(1 for g in got if g) > len(got) // 2, "the short queries find their docs"
    assert {len(q) for q in queries} >= set(EDGES)


@pytest.mark.parametrize("rows,last", [(1, 1025), (2, 513), (2, 4096), (1, 0)])
def test_one_workgroup_with_a_next_query_and_an_edge_length_last(env, big, rows, last):
    """B = grid + 1, 2 x grid + 1: one workgroup has a next query, all the others do not"""
    fpx, oracle, Pair, ctx = env
    p, allitems, rng, grid, queries, _, _ = big
    qs = list(queries[: rows * grid]) + [_query(np.random.default_rng(last + rows), allitems, 1, last)]
    got, st = p.check(qs, _opts(fpx))
    assert st.path_flags & 64, st.path_flags
    assert got[: rows * grid] == big[5][: rows * grid]


def test_three_threads_each_with_its_own_copy_of_the_batch(env, big):
    """overlapping launches take their queries without the counter and without the staggered start: every gridDim.x-th"""
    fpx, oracle, Pair, ctx = env
    p, allitems, rng, grid, queries, want, _ = big
    out, errs = [None] * 3, []

    def work(t):
        try:
            mine = [q.copy() for q in queries]
            for _ in range(2):
                out[t] = p.reader.search_batch(mine, _opts(fpx))
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for t in range(3):
        got, st = out[t]
        assert st.path_flags & 64, st.path_flags
        assert got == want, f"thread {t}: not the oracle's results"


def test_duplicates_on_both_sides_of_the_register_edges(env, big):
    """one hash twice, in rounds (0,1), (0,3), (1,2), (3,4), (3,8), (4,5) and (7,8) of a query of 2300 hashes (rounds 0 - 3 come from the
    registers the query started with, the later ones from the rolling window), 0xFFFFFFFF in rounds 0 and 3: a duplicate that is probed
    shows in the probes and in the scanned blocks"""
    fpx, oracle, Pair, ctx = env
    p, allitems, rng, grid, _, _, _ = big
    rng = np.random.default_rng(31)
    queries = []
    for v in range(3):
        q = rng.integers(0, 1 << 32, 2300, dtype=np.uint64).astype(np.uint32)
        src = allitems[v % len(allitems)]
        doc = src[rng.integers(0, len(src))] & np.uint64(0xFFFFFFFF)
        own = (src[(src & np.uint64(0xFFFFFFFF)) == doc] >> np.uint64(32)).astype(np.uint32)
        lanes = rng.permutation(250)[:8] if v else np.array([0, 63, 64, 255, 1, 128, 191, 100])
        for t, (r1, r2) in enumerate([(0, 1), (0, 3), (1, 2), (3, 4), (3, 8), (4, 5), (7, 8)]):
            q[r1 * 256 + lanes[t]] = own[t]
            q[r2 * 256 + (lanes[t] if v != 1 else lanes[(t + 1) % 7])] = own[t]
        q[0 * 256 + lanes[7]] = 0xFFFFFFFF
        q[3 * 256 + lanes[7]] = 0xFFFFFFFF
        q[2299] = own[8]                                          # (8 x 256 + 251: the last round's last lane with a hash)
        q[5] = own[8] if v == 2 else q[5]
        queries.append(q)
    got, st = p.check(queries, _opts(fpx))
    assert st.path_flags & 64, st.path_flags
    probes = 0
    for q in queries:
        _, ost = p.osnap.search(q, 100, 3, 10, with_stats=True)
        probes += ost.probes
    assert st.probes == probes, (st.probes, probes)
    assert all(g for g in got)


# ---- overflowing lines: a hash T in k columns, d of them doubles, behind n0 words of its line's first hashes -- n0 + k + d words is more
#      than a line holds inline (28 + the offset of the rest in `ext`): T's last words live in `ext`
def _overflow_cases(ncol):
    out = []
    for rep in range(3):
        for d in ((0, 5, 8) if ncol == 16 else (4, 6, 8)):
            for n0 in (19, 23, 27):
                out.append((ncol, d, n0 - (rep if n0 + ncol + d - rep > 29 else 0)))
    return out


def _overflow_world(fpx, Pair, ctx, monkeypatch, ncol, dead=False, per=600, seed=177):
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("group_packed", 1)
    try:
        rng = np.random.default_rng(seed + ncol)
        cases = _overflow_cases(ncol)
        firsts = [1 + s * per for s in range(ncol)]
        posts = [[] for _ in range(ncol)]

        def words(h, c, k, d):
            cols = sorted((c + i) % ncol for i in range(k))
            dbl = set(cols[(c + i) % k] for i in range(d))
            for s in cols:
                pool = firsts[s] + 10 + (np.arange(POOL) + c) % POOL
                posts[s].append((np.uint64(h) << np.uint64(32)) | pool[: 2 if s in dbl else 1].astype(np.uint64))

        targets = []
        for c, (k, d, n0) in enumerate(cases):
            t = BASE + c * 64 + (3 if ncol == 8 or c % 4 == 3 else 1)
            words(t, c, k, d)
            for off, n in ((0, min(n0, 2 * ncol)), (2, n0 - min(n0, 2 * ncol))):
                if n and BASE + c * 64 + off != t:
                    words(BASE + c * 64 + off, c + 1, min(n, ncol), max(0, n - ncol))
            targets.append(t)
        p = Pair(ctx)
        for s in range(ncol):
            docs = np.arange(firsts[s], firsts[s] + per, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (per, 24), dtype=np.uint64)
            items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel()] + posts[s]))
            p.add_file(items, firsts[s], firsts[s] + per - 1, s + 1, np.arange(firsts[s], firsts[s] + per, dtype=np.uint32))
        if dead:                                                  # one doc of every column's pool written again in a memory segment
            gone = [firsts[s] + 10 + s % POOL for s in range(ncol)]
            nxt = 1 + ncol * per
            ids = sorted(gone + list(range(nxt, nxt + 20)))
            h = rng.integers(0, 1 << 32, (len(ids), 24), dtype=np.uint64)
            items = np.unique(((h << np.uint64(32)) | np.asarray(ids, dtype=np.uint64)[:, None]).ravel())
            p.add_memory(items, ids[0], ids[-1], ncol + 1, np.asarray(ids, dtype=np.uint32))
        p.finish()
    finally:
        ctx.set_option("group_packed", -2)
    assert all(g.direct and g.grouped for g in p.gpu_segs[:ncol]), [g.layout_reason for g in p.gpu_segs[:ncol]]
    return p, np.asarray(targets, dtype=np.uint32), rng


def _overflow_queries(rng, targets):
    """queries of 1500 hashes (six rounds): overflowing hashes at lanes 0, 63, 64 and 255 of rounds 0, 1, 2, 3 and 5 -- the same lane in
    both rounds of a pair --, rotated through the cases; and short ones of a single case each"""
    qs = []
    for v in range(3):
        q = rng.integers(0, 1 << 32, 1500, dtype=np.uint64).astype(np.uint32)
        t = 9 * v
        for r in (0, 1, 2, 3, 5):
            for ln in (0, 63, 64, 255):
                if r * 256 + ln < len(q):
                    q[r * 256 + ln] = targets[t % len(targets)]
                    t += 1
        qs.append(q)
    for c in range(len(targets)):
        q = np.concatenate([targets[c:c + 1], targets[(c + 5) % len(targets)::11][:2], rng.integers(0, 1 << 32, 20 + c, dtype=np.uint64).astype(np.uint32)])
        qs.append(q)
    return qs


@pytest.mark.parametrize("ncol", [16, 8])
def test_overflowing_lines_in_every_round(env, ncol, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, targets, rng = _overflow_world(fpx, Pair, ctx, monkeypatch, ncol)
    queries = _overflow_queries(rng, targets)
    got, st = p.check(queries, fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0))
    assert st.path_flags & 64, st.path_flags
    assert all(len(g) > 1 for g in got[:3]), "the pools' docs reach the floor"


# ---- the other instantiations, a batch of 2 x grid + 3 queries of mixed lengths
def _mixed_batch(rng, allitems, grid):
    B = 2 * grid + 3
    lens = _mixed_lengths(rng, B, grid)
    return [_query(rng, allitems, i, int(n)) for i, n in enumerate(lens)]


def test_memory_segments_next_to_the_group(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, allitems, rng = _world(fpx, Pair, ctx, monkeypatch, 3, per=2000, memory=3)
    queries = _mixed_batch(rng, allitems, _grid())
    got, st = p.check(queries, _opts(fpx))
    assert st.path_flags & 64, st.path_flags
    assert any(g and g[0][0] > 6000 for g in got), "no query found its doc in a memory segment"


def test_filtered_form_with_a_dead_doc_in_every_column(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, targets, rng = _overflow_world(fpx, Pair, ctx, monkeypatch, 16, dead=True)
    grid = _grid()
    B = 2 * grid + 3
    lens = _mixed_lengths(rng, B, grid)
    queries = []
    for i, n in enumerate(lens):
        n = int(n)
        t = targets[rng.permutation(len(targets))[: min(n, 3 + i % 5)]]
        q = np.concatenate([t, rng.integers(0, 1 << 32, n - len(t), dtype=np.uint64).astype(np.uint32)])
        rng.shuffle(q)
        queries.append(q)
    gone = {1 + s * 600 + 10 + s % POOL for s in range(16)}
    ctx.set_option("query_wg", 2)
    try:
        got, st = p.check(queries, _opts(fpx))
        assert st.path_flags & 64, st.path_flags
        assert st.path_flags & 256, f"not the filtered form ({st.path_flags})"
        assert not gone & {r[0] for g in got for r in g}, "a superseded doc was returned"
    finally:
        ctx.set_option("query_wg", -1)


def test_per_query_statistics_of_a_workgroups_later_queries(env, big):
    """the statistics of every query of the large batch, asked for directly: a workgroup's second and third query write their own"""
    fpx, oracle, Pair, ctx = env
    p, allitems, rng, grid, queries, want, _ = big
    got, st, qb, qd = p.reader.search_batch_stats(queries, _opts(fpx))
    assert st.path_flags & 64 and got == want
    for i in list(range(0, len(queries), 97)) + [7 * j + 3 + grid for j in range(len(EDGES))] + [len(queries) - 1]:
        _, ost = p.osnap.search(queries[i], 100, 3, 10, with_stats=True)
        assert (int(qb[i]), int(qd[i])) == (ost.scanned_blocks, ost.scanned_docs), i
