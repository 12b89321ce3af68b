"""k_search_query's FILTERED form (csrc/fpx_qsearch.hpp, FILT; option query_wg = 2): a packed group whose snapshot holds superseded docs
(Index.update re-inserts a doc, a delete tombstones one: src/Index.zig:515-587) or columns outside the snapshot (merged away, not regrouped)
is still searched a query per workgroup.  Every word knows its column: a column outside the snapshot gives nothing, a doc a newer segment
supersedes is dropped after it was counted (src/common.zig:158).  Through Pair.check -- results and every query's scanned blocks / docs ==
the oracle's -- and against the pipeline (query_wg 0), which filters the same postings one by one (k_probe_pgroup).  path_flags bit 6: a
query per workgroup, bit 7: two parts, bit 8: the filtered form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHARED, MANY = 0x0BADF00D, 0x77770000


@pytest.fixture(scope="module")
def env():
    from fpx_testlib import fpx, oracle, Pair
    ctx = fpx.Context(0)
    yield fpx, oracle, Pair, ctx
    ctx.set_option("query_wg", -1)


def _rows(items, doc):
    return items[(items & np.uint64(0xFFFFFFFF)) == np.uint64(doc)]


def _col_items(rng, s, first, per):
    """a column's postings: 48 random hashes per doc, SHARED in a list of 2 / 3 / 4 / 70 / 5 docs, MANY a double in every column"""
    docs = np.arange(first, first + per, dtype=np.uint64)
    h = rng.integers(0, 1 << 32, (per, 48), dtype=np.uint64)
    parts = [((h << np.uint64(32)) | docs[:, None]).ravel(),
             (np.uint64(SHARED) << np.uint64(32)) | docs[: [2, 3, 4, 70, 5][s % 5]],
             (np.uint64(MANY) << np.uint64(32)) | docs[:2]]
    return np.unique(np.concatenate(parts))


def _queries(rng, allitems, n, qlen=1000, aim=()):
    """n queries of ~qlen hashes: a doc's own hashes + noise; `aim`: docs whose hashes (in the first items array that has them) lead"""
    qs = []
    for i in range(n):
        if i < len(aim):
            src = next(it for it in allitems if len(_rows(it, aim[i])))
            doc = aim[i]
        else:
            src = allitems[i % len(allitems)]
            doc = int(src[rng.integers(0, len(src))] & np.uint64(0xFFFFFFFF))
        own = (_rows(src, doc) >> np.uint64(32)).astype(np.uint32)
        extra = np.array([SHARED, MANY, SHARED], dtype=np.uint32)
        noise = rng.integers(0, 1 << 32, max(0, qlen - len(own) - len(extra)), dtype=np.uint64).astype(np.uint32)
        q = np.concatenate([own, extra, noise])
        rng.shuffle(q)
        qs.append(q)
    return qs


def _search(fpx, p, ctx, queries, opts, filt=True, parts=False):
    """query_wg 2 through Pair.check (the oracle), then query_wg 0: the same bytes, the same statistics"""
    ctx.set_option("query_wg", 2)
    try:
        got, st = p.check(queries, opts)
        assert st.path_flags & 64, f"not a query per workgroup ({st.path_flags})"
        assert bool(st.path_flags & 256) == filt, f"filtered form: want {filt} ({st.path_flags})"
        assert bool(st.path_flags & 128) == parts, f"two parts: want {parts} ({st.path_flags})"
        _, _, qb2, qd2 = p.reader.search_batch_stats(queries, opts)
    finally:
        ctx.set_option("query_wg", -1)
    ctx.set_option("query_wg", 0)
    try:
        got0, st0 = p.reader.search_batch(queries, opts)
        _, _, qb0, qd0 = p.reader.search_batch_stats(queries, opts)
    finally:
        ctx.set_option("query_wg", -1)
    assert not st0.path_flags & (64 | 128 | 256)
    assert got0 == got
    assert (st0.scanned_blocks, st0.scanned_docs) == (st.scanned_blocks, st.scanned_docs)
    if not parts:
        assert (st0.probes, st0.hits) == (st.probes, st.hits), ((st0.probes, st0.hits), (st.probes, st.hits))
    assert list(qb0) == list(qb2) and list(qd0) == list(qd2)
    return got, st


def _group(fpx, Pair, ctx, monkeypatch, rng, ncol, per, reinserts=None):
    """a packed group of ncol columns; reinserts: {column: [docs of older columns it writes again with their SAME hashes]}"""
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("group_packed", 1)
    p = Pair(ctx)
    allitems = []
    for s in range(ncol):
        first = s * per + 1
        items = _col_items(rng, s, first, per)
        ids = list(range(first, first + per))
        for d in (reinserts or {}).get(s, []):
            old = next(it for it in allitems if len(_rows(it, d)))
            items = np.unique(np.concatenate([items, _rows(old, d)]))
            ids.append(d)
        p.add_file(items, min(ids), max(ids), s + 1, np.array(sorted(ids), dtype=np.uint32))
        allitems.append(items)
    return p, allitems


def test_clean_group_under_2_takes_the_unfiltered_kernel(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8101)
    try:
        p, allitems = _group(fpx, Pair, ctx, monkeypatch, rng, 5, 2000)
        p.finish()
        assert all(g.grouped for g in p.gpu_segs)
        queries = _queries(rng, allitems, 24)
        got, _ = _search(fpx, p, ctx, queries, fpx.http_options(), filt=False)
        got1, st1 = p.reader.search_batch(queries, fpx.http_options())       # (query_wg 1: the default)
        assert st1.path_flags & 64 and not st1.path_flags & 256 and got1 == got
    finally:
        ctx.set_option("group_packed", -2)


def test_reinsert_with_new_hashes_in_a_memory_segment(env, monkeypatch):
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8102)
    per = 2500
    try:
        p, allitems = _group(fpx, Pair, ctx, monkeypatch, rng, 4, per)
        nxt, gone = 4 * per + 1, [17, 2 * per + 3, 3 * per + 40]              # (a plain doc, one in a list of 4, one in a list of 70)
        for m in range(4):
            docs = np.arange(nxt, nxt + 50, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (50, 40), dtype=np.uint64)
            items = [((h << np.uint64(32)) | docs[:, None]).ravel()]
            ids = list(range(nxt, nxt + 50))
            if m == 1:
                for d in gone:                                           # written again, with other hashes
                    items.append((rng.integers(0, 1 << 32, 40, dtype=np.uint64) << np.uint64(32)) | np.uint64(d))
                    ids.append(d)
            items = np.unique(np.concatenate(items))
            p.add_memory(items, min(ids), max(ids), 5 + m, np.array(sorted(ids), dtype=np.uint32))
            allitems.append(items)
            nxt += 50
        p.finish()
        queries = _queries(rng, allitems, 30, aim=gone)                  # (the first three: the OLD hashes of the re-inserted docs)
        for opts in (fpx.http_options(), fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)):
            got, st = _search(fpx, p, ctx, queries, opts)
        assert all(d not in [r[0] for r in got[i]] for i, d in enumerate(gone)), "a superseded doc was returned"
    finally:
        ctx.set_option("group_packed", -2)


def test_reinsert_with_the_same_hashes_inside_the_group(env, monkeypatch):
    """9 columns (lines of 4 hash values): the newest column writes again, with their SAME hashes, a plain doc of column 0, a doc in
    column 2's list of four SHARED docs (a list head), one in column 3's list of 70 (read on by the wave), and a MANY doc of column 6 --
    MANY is a double in every column: 18 words, of which those of columns 6 .. 8 are a words task beyond the lane's twelve"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8103)
    per = 1500
    again = [17, 2 * per + 2, 3 * per + 5, 6 * per + 1]
    try:
        p, allitems = _group(fpx, Pair, ctx, monkeypatch, rng, 9, per, reinserts={8: again})
        p.finish()
        assert all(g.grouped for g in p.gpu_segs), [g.layout_reason for g in p.gpu_segs]
        queries = _queries(rng, allitems, 36, aim=again)
        for opts in (fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0)):
            got, st = _search(fpx, p, ctx, queries, opts)
        for i, d in enumerate(again):
            assert got[i] and got[i][0][0] == d and [r[0] for r in got[i]].count(d) == 1, (d, got[i][:4])
    finally:
        ctx.set_option("group_packed", -2)


def test_tombstones_and_checkpoints_in_two_parts(env, monkeypatch):
    """deletes of group docs (MemorySegment changes), a checkpoint in blocks that tombstones a group doc (the seed-3 shape of
    test_random_live_worlds_in_two_parts) and one that re-inserts one: made under query_wg 2, the snapshot is searched in two parts with
    the filtered form on part 0 -- whose dead sets hold the docs of part 1 and of the memory segments"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8104)
    per = 2000
    try:
        p, allitems = _group(fpx, Pair, ctx, monkeypatch, rng, 4, per)
        p.finish()
        assert all(g.grouped for g in p.gpu_segs)
        nxt, commit = 4 * per + 1, 5
        ctx.set_option("direct_min_items", 1 << 20)                       # checkpoints, in blocks
        for s in range(3):
            docs = np.arange(nxt, nxt + 600, dtype=np.uint64)
            ids, alive = list(range(nxt, nxt + 600)), [1] * 600
            h = rng.integers(0, 1 << 32, (600, 40), dtype=np.uint64)
            parts = [((h << np.uint64(32)) | docs[:, None]).ravel(), (np.uint64(SHARED) << np.uint64(32)) | docs[:6]]
            if s == 0:
                ids.insert(0, 5); alive.insert(0, 0)                       # doc 5 of the group: a tombstone
            if s == 1:
                parts.append(_rows(allitems[1], per + 9)); ids.append(per + 9); alive.append(1)     # ... and doc per + 9 written again
            order = np.argsort(ids)
            items = np.unique(np.concatenate(parts))
            p.add_file(items, min(ids), max(ids), commit, np.array(ids, dtype=np.uint32)[order], np.array(alive, dtype=np.uint8)[order])
            allitems.append(items)
            nxt += 600; commit += 1
        ctx.set_option("direct_min_items", -1)
        p.add_memory_changes([("delete", 2 * per + 1), ("delete", 3 * per + 7), ("insert", nxt, rng.integers(0, 1 << 32, 30).tolist())], commit)
        ctx.set_option("query_wg", 2)                                     # (the value in force when the snapshot is made)
        try:
            p.finish()
        finally:
            ctx.set_option("query_wg", -1)
        queries = _queries(rng, allitems, 33, aim=[5, per + 9, 2 * per + 1, 3 * per + 7])
        got_http, _ = _search(fpx, p, ctx, queries, fpx.http_options(), parts=True)
        got, st = _search(fpx, p, ctx, queries, fpx.SearchOptions(max_results=60, min_score=4, min_score_pct=30), parts=True)
        assert not any(r[0] in (5, 2 * per + 1, 3 * per + 7) for g in got + got_http for r in g), "a deleted doc was returned"
        # under query_wg 1 the same snapshot keeps today's routing: one part, the pipeline
        got1, st1 = p.reader.search_batch(queries, fpx.http_options())
        assert not st1.path_flags & (64 | 128 | 256) and got1 == got_http
    finally:
        ctx.set_option("group_packed", -2); ctx.set_option("direct_min_items", -1)


def _merged_world(fpx, oracle, Pair, ctx, monkeypatch, rng, mem, dead):
    """four columns in a packed group, the two oldest merged (a segment of its own next to the group, no regroup): the group keeps two
    columns outside the snapshot"""
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("direct_min_items", 0)
    ctx.set_option("group_packed", 1)
    p = Pair(ctx)
    raw = []
    for s in range(4):
        ids = np.arange(s * 2000 + 1, (s + 1) * 2000 + 1)
        items = _col_items(rng, s, s * 2000 + 1, 2000)
        p.add_file(items, int(ids.min()), int(ids.max()), s + 1, ids.astype(np.uint32))
        raw.append(items)
    p.finish()
    assert all(g.grouped for g in p.gpu_segs)
    merged = p.reader.snapshot.merge(p.gpu_segs[0:2], 512)
    want = p.osnap.merge(p.orc_file[0:2])
    wb, wi = oracle.build_blocks(want["items"], want["min_doc_id"], 512)
    q = Pair(ctx)
    q.gpu_segs = [merged] + p.gpu_segs[2:]
    q.orc_file = [oracle.file_segment(wb, 512, wi, want["min_doc_id"], want["max_doc_id"], want["commit_id"], want["doc_ids"], want["doc_alive"])] + p.orc_file[2:]
    if mem:
        nxt = 8001
        for m in range(2):
            docs = np.arange(nxt, nxt + 40, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (40, 30), dtype=np.uint64)
            parts = [((h << np.uint64(32)) | docs[:, None]).ravel()]
            ids = list(range(nxt, nxt + 40))
            if dead and m == 1:
                parts.append(_rows(raw[2], 4003)); ids.append(4003)          # a doc of an active column written again
            items = np.unique(np.concatenate(parts))
            q.add_memory(items, min(ids), max(ids), 10 + m, np.array(sorted(ids), dtype=np.uint32))
            raw.append(items)
            nxt += 40
    elif dead:
        q.add_memory_changes([("delete", 6001), ("insert", 8001, rng.integers(0, 1 << 32, 30).tolist())], 10)
    ctx.set_option("query_wg", 2)
    try:
        q.finish()
    finally:
        ctx.set_option("query_wg", -1)
    return q, raw


@pytest.mark.parametrize("mem,dead", [(False, False), (True, False), (False, True), (True, True)])
def test_masked_columns_after_a_merge_without_regroup(env, monkeypatch, mem, dead):
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8105 + 2 * mem + dead)
    try:
        q, raw = _merged_world(fpx, oracle, Pair, ctx, monkeypatch, rng, mem, dead)
        info = q.reader.snapshot.info()
        assert info["groups"] == 1, info
        queries = _queries(rng, raw, 30, aim=[17, 2500, 4003, 6001])     # (docs of the merged columns, of both active ones)
        for opts in (fpx.http_options(), fpx.SearchOptions(max_results=80, min_score=3, min_score_pct=0)):
            got, st = _search(fpx, q, ctx, queries, opts, parts=True)
        assert got[0] and got[0][0][0] == 17 and got[1] and got[1][0][0] == 2500     # (found in the merged segment, once)
    finally:
        ctx.set_option("group_packed", -2); ctx.set_option("direct_min_items", -1)


def test_hot_hashes_in_a_filtered_world_go_back_to_the_pipeline(env, monkeypatch):
    """a query of twelve hashes of 1000+ docs each outgrows the LDS records: the filtered form hands the batch back (CTR_BINFAIL) too"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(8106)
    per = 4000
    hots = [0x40000000 + 977 * k for k in range(12)]
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("group_packed", 1)
    try:
        p = Pair(ctx)
        allitems = []
        for s in range(3):
            first = s * per + 1
            docs = np.arange(first, first + per, dtype=np.uint64)
            ids = list(range(first, first + per)) + ([11] if s == 2 else [])
            h = rng.integers(0, 1 << 32, (per, 48), dtype=np.uint64)
            items = [((h << np.uint64(32)) | docs[:, None]).ravel()] + [(np.uint64(k) << np.uint64(32)) | docs[:1500] for k in hots[s::3]]
            if s == 2:
                items.append(_rows(allitems[0], 11))                              # doc 11 written again: column 0 has a dead set
            items = np.unique(np.concatenate(items))
            p.add_file(items, min(ids), max(ids), s + 1, np.array(sorted(ids), dtype=np.uint32))
            allitems.append(items)
        p.finish()
        assert all(g.grouped for g in p.gpu_segs)
        plain = _queries(rng, allitems, 16, aim=[11])
        _search(fpx, p, ctx, plain, fpx.http_options())
        heavy = list(plain)
        heavy[5] = np.concatenate([plain[5][:900], np.array(hots, dtype=np.uint32)])
        ctx.set_option("query_wg", 2)
        try:
            got_h, st_h = p.reader.search_batch(heavy, fpx.http_options())
        finally:
            ctx.set_option("query_wg", -1)
        assert not st_h.path_flags & (64 | 256), "12 x 1000+ records fit 8192?"
        for qq, g in zip(heavy, got_h):
            assert g == p.osnap.search(qq, 40, None, 10)
    finally:
        ctx.set_option("group_packed", -2)
