"""Doc ids at the top of the u32 range, across 2^31 and at every threshold the ids decide.  Ids are u32 in the reference, 0 is
reserved and 1 .. 0xFFFFFFFF are all legal (src/MultiIndex.zig:333-342); the library chooses storage forms and record widths by
how large and how widely spread they are:

* a segment spanning 2^31 or more has no direct-addressed form (fpx_build.hip: direct_candidate);
* a group spanning 0x7FFFFFF0 or more has no packed form (fpx_group.hip: its words count from one base);
* words hold doc - base in 31 bits, bit 31 tags a list: the largest legal word is 0x7FFFFFFF (direct) / 0x7FFFFFEF (packed);
* a dead set whose ids span 2^29 or more has no bitmap: every probe kernel searches the sorted list (is_dead);
* bins of 2^bq queries hold 4-byte records (doc << bq | query) only while the declared max doc is below 0xFFFFFFFF >> bq;
* results are ordered (score desc, id asc) -- k_finish and k_merge key on ~id.

Every case is legal input on one side of a threshold, is compared with the oracle through Pair.check (results, per-query scanned
blocks / docs, the device-sized repeat, search_batch_stats) and asserts the form and path it was built for, so that a later
change of a threshold cannot move it to another path unnoticed.  The docs at the extreme ids sit in single words, doubles,
lists of 3 / 5 / 70 docs and a hash of 3000 docs (the reference's 4-block / 1000-doc caps), and the queries aim at them."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF
SIGN = 0x80000000
H = 24                                                   # random hashes per doc
DOUBLE, L3, L5, L70, HOT = 0x0D0B1E00, 0x0BADF003, 0x0BADF005, 0x0BADF070, 0x12345678
TIE = 0x7E700000                                          # TIE + k, k < 30: hashes the tie docs share


@pytest.fixture(scope="module")
def env():
    from fpx_testlib import fpx, oracle, Pair
    ctx = fpx.Context(0)
    yield fpx, oracle, Pair, ctx
    _reset(ctx)


def _reset(ctx):
    for name in ("fuse_min", "query_wg", "rec32", "lean_min", "direct_min_items", "presence_min_items"):
        ctx.set_option(name, -1)
    ctx.set_option("group_packed", -2)


def _options(fpx):
    """the option sets every case runs: the HTTP defaults (floor = len / 20), a wide explicit floor, a limit inside the ranking"""
    return [fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0),
            fpx.SearchOptions(max_results=2, min_score=5, min_score_pct=50)]


@pytest.fixture
def fresh(env, monkeypatch):
    """each test starts from the defaults, with every file segment a direct-addressed candidate (FPX_DIRECT_MIN_ITEMS=0)"""
    fpx, oracle, Pair, ctx = env
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    _reset(ctx)
    yield ctx
    _reset(ctx)
    gc.collect()


def _items(rng, docs, marked, hot=False):
    """postings of `docs`: H random hashes per doc (single words), and around the `marked` docs the rare shapes -- a double of
    two marked docs and one of a marked doc with another, lists of 3, 5 and 70 docs and (hot) a hash of 3000 docs that hold them"""
    docs = np.asarray(docs, np.uint64)
    marked = np.asarray(marked, np.uint64)
    others = docs[~np.isin(docs, marked)]
    h = rng.integers(0, 1 << 32, (len(docs), H), dtype=np.uint64)
    parts = [((h << np.uint64(32)) | docs[:, None]).ravel()]

    def post(hash_, ids):
        parts.append((np.uint64(hash_) << np.uint64(32)) | np.asarray(ids, np.uint64))

    def pick(n):                                          # the marked docs + the others nearest the top of the column
        m = marked[:n]
        return np.concatenate([m, others[len(others) - (n - len(m)):]]) if n > len(m) else m

    if len(marked) >= 2:
        post(DOUBLE, marked[:2])
    post(DOUBLE + 1, [marked[-1], others[0]])
    post(L3, pick(3)); post(L5, pick(5)); post(L70, pick(70))
    if hot:
        post(HOT, pick(3000))
    return np.unique(np.concatenate(parts))


def _rows(items, doc):
    return items[(items & np.uint64(0xFFFFFFFF)) == np.uint64(doc)]


def _queries(rng, allitems, aim, n, qlen=120):
    """n queries: the first aim at the `aim` docs (their own hashes, rare shapes included, + noise), the rest at random docs"""
    qs = []
    for i in range(n):
        if i < len(aim):
            own = np.concatenate([_rows(it, aim[i]) for it in allitems])
            assert len(own), hex(aim[i])
        else:
            src = allitems[i % len(allitems)]
            own = _rows(src, int(src[rng.integers(0, len(src))] & np.uint64(0xFFFFFFFF)))
        own = np.unique((own >> np.uint64(32)).astype(np.uint32))
        noise = rng.integers(0, 1 << 32, max(0, qlen - len(own)), dtype=np.uint64).astype(np.uint32)
        q = np.concatenate([own, noise])
        rng.shuffle(q)
        qs.append(q)
    return qs


def _check(fpx, p, queries, want_flags=0, not_flags=0, options=None):
    """Pair.check under every option set; the path bits `want_flags` set and `not_flags` clear on each; the results"""
    res = []
    for o in options or _options(fpx):
        got, st = p.check(queries, o)
        assert st.path_flags & want_flags == want_flags and not st.path_flags & not_flags, (st.path_flags, want_flags, not_flags)
        res.append(got)
    return res


def _found(got, docs):
    """every one of `docs` is the first result of the query aimed at it"""
    for i, d in enumerate(docs):
        assert got[i] and got[i][0][0] == d, (hex(d), got[i][:3])


def _single(fpx, p, queries):
    """the single-query entry point (fpx_search, B = 1) on the same queries"""
    for q in queries:
        for o in _options(fpx):
            r = fpx.SearchResults(o)
            p.reader.search(q, r)
            assert r.getResults() == p.osnap.search(q, o.max_results, o.min_score, o.min_score_pct), hex(q[0])


def _file(p, rng, docs, marked, commit, hot=False, block_size=512, alive=None):
    items = _items(rng, docs, marked, hot)
    docs = np.asarray(docs, np.uint64)
    p.add_file(items, int(docs.min()), int(docs.max()), commit, docs.astype(np.uint32), alive, block_size=block_size)
    return items


def _group(fpx, Pair, ctx, rng, columns, marked, packed, hot=True):
    """a group of direct-addressed file segments, one per entry of `columns` (doc id arrays), in the packed form or not"""
    ctx.set_option("group_packed", 1 if packed else 0)
    p = Pair(ctx)
    allitems = [_file(p, rng, docs, [m for m in marked if m in set(int(x) for x in docs)] or [int(docs[-1])], s + 1, hot=hot and s == 0)
                for s, docs in enumerate(columns)]
    p.finish()
    assert all(g.direct and g.grouped for g in p.gpu_segs), [g.layout_reason for g in p.gpu_segs]
    info = p.gpu_segs[0].group_info()
    assert info["columns"] == len(columns) and info["packed"] == int(packed), info
    return p, allitems


def _span(lo, n):
    return np.arange(lo, lo + n, dtype=np.uint64)


# ---- a. the top of the range on every form ---------------------------------------------------------------------------------

TOP_MARKED = [TOP - 1, TOP]


@pytest.mark.parametrize("block_size", [64, 512, 4096])
@pytest.mark.parametrize("lean", [1, 0])
def test_top_of_the_range_in_blocks(env, fresh, block_size, lean):
    """a segment in blocks ending at 0xFFFFFFFF, searched by the lean / small kernels (lean_min 0) and by the generic one"""
    fpx, oracle, Pair, ctx = env
    ctx.set_option("direct_min_items", 1 << 40)
    ctx.set_option("lean_min", 0 if lean else 1 << 40)
    rng = np.random.default_rng(7100 + block_size + lean)
    p = Pair(ctx)
    docs = _span(TOP - 3999, 4000)
    items = [_file(p, rng, docs, TOP_MARKED, 1, hot=True, block_size=block_size)]
    p.finish()
    info = p.reader.snapshot.info()
    assert not p.gpu_segs[0].direct and info["block_form_files"] == 1 and info["lean"] + info["generic"] + info["small"] == 1, info
    queries = _queries(rng, items, TOP_MARKED + [TOP - 2], 24)
    got = _check(fpx, p, queries, not_flags=4 | 64)
    _found(got[0], TOP_MARKED + [TOP - 2])
    _single(fpx, p, queries[:3])


def test_top_of_the_range_lean_sized(env, fresh):
    """2^20 + items in 512-byte blocks: the lean kernel proper (presence bits, probe records) against the generic one"""
    fpx, oracle, Pair, ctx = env
    ctx.set_option("direct_min_items", 1 << 40)
    rng = np.random.default_rng(7110)
    p = Pair(ctx)
    docs = _span(TOP - 9999, 10000)
    items = _items(rng, docs, TOP_MARKED, hot=True)
    extra = rng.integers(0, 1 << 32, (len(docs), 90), dtype=np.uint64)
    items = np.unique(np.concatenate([items, ((extra << np.uint64(32)) | docs[:, None]).ravel()]))
    assert len(items) >= 1 << 20
    p.add_file(items, int(docs[0]), TOP, 1, docs.astype(np.uint32))
    p.finish()
    assert p.reader.snapshot.info()["lean"] == 1, p.reader.snapshot.info()
    queries = _queries(rng, [items], TOP_MARKED, 600, qlen=200)
    res = {}
    for lean in (1, 0):
        ctx.set_option("lean_min", 0 if lean else 1 << 40)
        res[lean] = _check(fpx, p, queries, options=_options(fpx)[:2])
    assert res[0] == res[1]
    _found(res[1][0], TOP_MARKED)


def test_top_of_the_range_direct_alone(env, fresh):
    fpx, oracle, Pair, ctx = env
    ctx.set_option("fuse_min", 0)
    rng = np.random.default_rng(7120)
    p = Pair(ctx)
    items = [_file(p, rng, _span(TOP - 3999, 4000), TOP_MARKED, 1, hot=True)]
    p.finish()
    s = p.gpu_segs[0]
    assert s.direct and not s.grouped and p.reader.snapshot.info()["direct_solo"] == 1, s.layout_reason
    queries = _queries(rng, items, TOP_MARKED + [TOP - 2], 24)
    got = _check(fpx, p, queries, not_flags=4 | 64)
    _found(got[0], TOP_MARKED)
    _single(fpx, p, queries[:3])


@pytest.mark.parametrize("packed", [0, 1])
def test_top_of_the_range_in_a_group(env, fresh, packed):
    """three columns ending at 0xFFFFFFFF: directory + words (k_probe_group), packed through the pipeline (query_wg 0) and a query
    per workgroup (k_search_query, bit 6)"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7130 + packed)
    cols = [_span(TOP - 3 * 3200 + 1 + c * 3200, 3200) for c in range(3)]
    p, items = _group(fpx, Pair, ctx, rng, cols, TOP_MARKED + [int(cols[0][0]), int(cols[0][-1])], packed)
    queries = _queries(rng, items, TOP_MARKED + [int(cols[0][0])], 32)
    ctx.set_option("query_wg", 0)
    got0 = _check(fpx, p, queries, want_flags=4, not_flags=64)
    _found(got0[0], TOP_MARKED + [int(cols[0][0])])
    ctx.set_option("query_wg", -1)
    if packed:
        got1 = _check(fpx, p, queries, want_flags=64)
        assert got1 == got0
    _single(fpx, p, queries[:3])


def test_top_of_the_range_memory_next_to_a_packed_group(env, fresh):
    """a memory segment holding the top docs next to a packed group: k_search_query's MEM instantiation (bit 6), and the pipeline"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7140)
    cols = [_span(TOP - 100 - 2 * 3000 + 1 + c * 3000, 3000) for c in range(2)]
    p, items = _group(fpx, Pair, ctx, rng, cols, [int(cols[1][-1])], True)
    mdocs = _span(TOP - 99, 100)
    mitems = _items(rng, mdocs, TOP_MARKED)
    p.add_memory(mitems, int(mdocs[0]), TOP, 3, mdocs.astype(np.uint32))
    p.finish()
    info = p.reader.snapshot.info()
    assert info["memory"] == 1 and info["packed_groups"] == 1, info
    queries = _queries(rng, items + [mitems], TOP_MARKED + [int(cols[1][-1])], 32)
    got1 = _check(fpx, p, queries, want_flags=64, not_flags=128)
    _found(got1[0], TOP_MARKED + [int(cols[1][-1])])
    ctx.set_option("query_wg", 0)
    assert _check(fpx, p, queries, not_flags=64) == got1
    ctx.set_option("query_wg", -1)
    _single(fpx, p, queries[:3])


# ---- b. across the sign bit --------------------------------------------------------------------------------------------------

SIGN_MARKED = [SIGN - 1, SIGN, 0x7FFFF000, 0x80000FFF]


@pytest.mark.parametrize("form", ["blocks", "direct"])
def test_across_the_sign_bit_in_one_segment(env, fresh, form):
    fpx, oracle, Pair, ctx = env
    if form == "blocks":
        ctx.set_option("direct_min_items", 1 << 40)
    else:
        ctx.set_option("fuse_min", 0)
    rng = np.random.default_rng(7200 + (form == "direct"))
    p = Pair(ctx)
    items = [_file(p, rng, _span(0x7FFFF000, 0x2000), SIGN_MARKED, 1, hot=True)]
    p.finish()
    assert p.gpu_segs[0].direct == (form == "direct") and not p.gpu_segs[0].grouped, p.gpu_segs[0].layout_reason
    queries = _queries(rng, items, SIGN_MARKED, 24)
    got = _check(fpx, p, queries, not_flags=4 | 64)
    _found(got[0], SIGN_MARKED)


@pytest.mark.parametrize("packed", [0, 1])
def test_across_the_sign_bit_over_the_columns_of_a_group(env, fresh, packed):
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7210 + packed)
    cols = [_span(0x7FFFF000 + c * 0x800, 0x800) for c in range(4)]              # column 1 ends at 2^31 - 1, column 2 starts at 2^31
    p, items = _group(fpx, Pair, ctx, rng, cols, SIGN_MARKED, packed, hot=False)
    queries = _queries(rng, items, SIGN_MARKED, 24)
    ctx.set_option("query_wg", 0)
    got0 = _check(fpx, p, queries, want_flags=4, not_flags=64)
    _found(got0[0], SIGN_MARKED)
    ctx.set_option("query_wg", -1)
    if packed:
        assert _check(fpx, p, queries, want_flags=64) == got0


# ---- c. each threshold from both sides ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("span", [(1 << 31) - 1, 1 << 31])
def test_direct_form_threshold(env, fresh, span):
    """a segment of two clusters, min = 0xFFFFFFFF - span: span 2^31 - 1 is direct-addressed and stores the word 0x7FFFFFFF for doc
    0xFFFFFFFF; span 2^31 stays in its blocks"""
    fpx, oracle, Pair, ctx = env
    ctx.set_option("fuse_min", 0)
    rng = np.random.default_rng(7300 + (span >> 31))
    lo = TOP - span
    docs = np.concatenate([_span(lo, 1500), _span(TOP - 1499, 1500)])
    marked = [lo, lo + 1, TOP - 1, TOP]
    p = Pair(ctx)
    items = [_file(p, rng, docs, marked, 1)]
    p.finish()
    s = p.gpu_segs[0]
    if span < 1 << 31:
        assert s.direct and not s.grouped, s.layout_reason
    else:
        assert not s.direct and "spanning 2^31" in s.layout_reason, s.layout_reason
    queries = _queries(rng, items, marked, 24)
    got = _check(fpx, p, queries, not_flags=4 | 64)
    _found(got[0], marked)
    _single(fpx, p, queries[:4])


@pytest.mark.parametrize("span", [0x7FFFFFEF, 0x7FFFFFF0])
def test_packed_form_threshold(env, fresh, span):
    """a group of two columns, gmin = 0xFFFFFFFF - span: span 0x7FFFFFEF is packed (its largest word, 0x7FFFFFEF, is doc
    0xFFFFFFFF) and runs k_search_query; span 0x7FFFFFF0 is directory + words even with group_packed 1"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7310 + (span & 1))
    gmin = TOP - span
    cols = [_span(gmin, 2500), _span(TOP - 2499, 2500)]
    marked = [gmin, gmin + 1, TOP - 1, TOP]
    ctx.set_option("group_packed", 1)
    p = Pair(ctx)
    items = [_file(p, rng, cols[0], marked[:2], 1, hot=False), _file(p, rng, cols[1], marked[2:], 2)]
    p.finish()
    assert all(g.direct and g.grouped for g in p.gpu_segs), [g.layout_reason for g in p.gpu_segs]
    packed = span < 0x7FFFFFF0
    assert p.gpu_segs[0].group_info()["packed"] == int(packed), p.gpu_segs[0].group_info()
    queries = _queries(rng, items, marked, 24)
    got = _check(fpx, p, queries, want_flags=(64 if packed else 4), not_flags=(0 if packed else 64))
    _found(got[0], marked)
    if packed:
        ctx.set_option("query_wg", 0)
        assert _check(fpx, p, queries, want_flags=4, not_flags=64) == got


# ---- d. ties across 2^31 and at 0xFFFFFFFF, cut by the limit -----------------------------------------------------------------

TIES = [3, SIGN - 1, SIGN, TOP]


def _tie_world(fpx, Pair, ctx, rng):
    """a packed group (columns around 2^31: docs 2^31 - 1 and 2^31), a checkpoint file segment in blocks (doc 3) and a memory
    segment (doc 0xFFFFFFFF); the four tie docs share the thirty TIE hashes"""
    tie = (np.uint64(TIE) + np.arange(30, dtype=np.uint64)) << np.uint64(32)
    ctx.set_option("group_packed", 1)
    p = Pair(ctx)
    raw = []
    for s, docs in enumerate([_span(SIGN - 0x800, 0x800), _span(SIGN, 0x800)]):
        it = np.unique(np.concatenate([_items(rng, docs, [d for d in TIES if d in (int(docs[0]), int(docs[-1]))] or [int(docs[-1])]),
                                       tie | np.uint64(TIES[1 + s])]))
        p.add_file(it, int(docs[0]), int(docs[-1]), s + 1, docs.astype(np.uint32))
        raw.append(it)
    p.finish()                                                                    # (the group forms when a snapshot first holds it)
    ctx.set_option("direct_min_items", 1 << 40)                                   # the checkpoint stays in blocks
    docs = _span(1, 1500)
    it = np.unique(np.concatenate([_items(rng, docs, [3]), tie | np.uint64(3)]))
    p.add_file(it, 1, 1500, 3, docs.astype(np.uint32))
    raw.append(it)
    mdocs = _span(TOP - 49, 50)
    it = np.unique(np.concatenate([_items(rng, mdocs, [TOP]), tie | np.uint64(TOP)]))
    p.add_memory(it, int(mdocs[0]), TOP, 4, mdocs.astype(np.uint32))
    raw.append(it)
    p.finish()
    assert p.gpu_segs[0].grouped and p.gpu_segs[0].group_info()["packed"] == 1 and not p.gpu_segs[2].direct
    return p, raw


def test_ties_across_two_parts_and_the_limit(env, fresh):
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7400)
    p, raw = _tie_world(fpx, Pair, ctx, rng)
    tie = np.arange(TIE, TIE + 30, dtype=np.uint32)
    queries = []
    for i in range(16):
        noise = rng.integers(0, 1 << 32, 40 + 7 * i, dtype=np.uint64).astype(np.uint32)
        q = np.concatenate([tie, noise])
        rng.shuffle(q)
        queries.append(q)
    queries += _queries(rng, raw, TIES, 8)
    cuts = [fpx.SearchOptions(max_results=k, min_score=3, min_score_pct=10) for k in (1, 2, 3, 4, 5)] + [fpx.http_options(limit=2)]
    res = {}
    for qwg in (1, 0):
        ctx.set_option("query_wg", qwg)
        res[qwg] = _check(fpx, p, queries, want_flags=(128 | 64) if qwg else 0, not_flags=0 if qwg else 64 | 128, options=cuts)
    assert res[0] == res[1]
    for k, got in zip((1, 2, 3, 4, 5), res[1]):
        assert [r[0] for r in got[0]] == TIES[:k], (k, got[0])
        assert all(r[1] == 30 for r in got[0][:min(k, 4)])
    ctx.set_option("query_wg", -1)
    # the same tie through segment sharding: whole segments per rank, docs-only stand-ins, per-rank tables merged (fpx_merge_partials)
    import torch
    ctx.set_option("direct_min_items", 1 << 40)
    world, mem = 3, p.gpu_segs[-1]
    readers = []
    for r in range(world):
        segs = []
        for s, g in enumerate(p.gpu_segs[:3]):
            ids, alive = g.docs()
            if s % world == r:
                blocks, index = oracle.build_blocks(raw[s], g.min_doc_id, 512)
                segs.append(fpx.FileSegment(ctx, blocks, 512, index, g.min_doc_id, g.max_doc_id, g.commit_id, ids, alive))
            else:
                segs.append(fpx.RemoteSegment(ctx, g.min_doc_id, g.max_doc_id, g.commit_id, ids, alive))
        segs.append(fpx.MemorySegment(ctx, raw[3], mem.min_doc_id, mem.max_doc_id, mem.commit_id, mem.doc_ids, mem.doc_alive)
                    if r == world - 1 else fpx.RemoteSegment(ctx, mem.min_doc_id, mem.max_doc_id, mem.commit_id, mem.doc_ids, mem.doc_alive))
        readers.append(fpx.IndexReader(fpx.Segments(ctx, segs)))
    for o, want in zip(cuts, res[1]):
        qb = fpx.QueryBatch(ctx, queries, o)
        parts = torch.zeros((world, qb.B, qb.cap, 2), dtype=torch.int32, device="cuda")
        cnts = torch.zeros((world, qb.B), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()            # (torch fills on ITS stream; libfpx writes these on a stream of its own)
        for r in range(world):
            fpx.search_resident_partial(readers[r], qb, parts[r].data_ptr(), cnts[r].data_ptr())
        torch.cuda.synchronize()
        out, out_n = fpx.merge_partials(ctx, qb, parts.data_ptr(), cnts.data_ptr(), world)
        assert fpx.results_to_lists(out, out_n) == want, o


# ---- e. dead sets wider than 2^29: the sorted-list search ----------------------------------------------------------------------

def _dead_changes(rng, lo_doc, hi_doc, wide):
    """a newer memory segment: deletes at both ends of an older segment's range (or, narrow, both near its low end) and a
    re-insert with new hashes"""
    ends = [lo_doc + 4, hi_doc - 3] if wide else [lo_doc + 4, lo_doc + 9]
    return [("delete", ends[0]), ("insert", ends[1], rng.integers(0, 1 << 32, 30).tolist()), ("delete", lo_doc + 30)], ends


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("form", ["blocks", "direct", "words", "packed", "filtered", "two_parts"])
def test_dead_sets_wider_than_2_29(env, fresh, form, wide):
    """an older segment of two clusters (span >= 2^29 and < 0x7FFFFFF0; in blocks: docs 1 .. 0xF0000000 and the top 100); a newer
    memory segment deletes / re-inserts docs at its two ends (wide: the sorted-list search) or near one end (narrow: the bitmap); the
    wide blocks world also deletes 0xFFFFFFFF.  Queries aim at the deleted and re-inserted docs' old hashes (their old postings must
    be dropped), at the re-inserted doc's new hashes (the memory segment's) and at live docs inside the dead range.
    (Which of the two searches a dead set gets is not visible through the API: the ids' range decides it, 2^29 or more here on the
    wide side -- an is_dead that takes any doc inside the range for dead makes exactly the wide cases fail, the narrow ones pass.)"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7500 + 2 * ["blocks", "direct", "words", "packed", "filtered", "two_parts"].index(form) + wide)
    lo, hi = (5, 0xF0000000) if form == "blocks" else (0x90000000, 0xE0000FFF)
    old = np.concatenate([_span(lo - 4, 1500), _span(hi - 1499, 1500)] + ([_span(TOP - 99, 100)] if form == "blocks" else []))
    changes, ends = _dead_changes(rng, lo - 4, hi, wide)
    if form == "blocks" and wide:
        changes.append(("delete", TOP))
        ends = ends + [TOP]
    grouped = form in ("words", "packed", "filtered", "two_parts")
    if form == "blocks":
        ctx.set_option("direct_min_items", 1 << 40)
    if not grouped:
        ctx.set_option("fuse_min", 0)
    ctx.set_option("group_packed", 0 if form == "words" else 1)
    p = Pair(ctx)
    marked = [int(old[0]), int(old[4]), int(old[1500]), int(old[1500 + 1496])]
    raw = [_file(p, rng, old, [m for m in marked], 1, hot=True)]
    if grouped:
        raw.append(_file(p, rng, _span(hi + 1, 2000), [hi + 1], 2))
    if form == "two_parts":
        p.finish()                                                                # (the group forms when a snapshot first holds it)
        ctx.set_option("direct_min_items", 1 << 40)
        raw.append(_file(p, rng, _span(0x40000000, 1200), [0x40000000], 3))       # a checkpoint in blocks
    p.add_memory_changes(changes, 9)
    ctx.set_option("query_wg", 2 if form in ("filtered", "two_parts") else 1)
    p.finish()
    s = p.gpu_segs[0]
    assert s.direct == (form != "blocks") and s.grouped == grouped, s.layout_reason
    if grouped:
        assert s.group_info()["packed"] == int(form != "words"), s.group_info()
    live = [int(old[1]), int(old[2000])]
    queries = _queries(rng, raw, ends + live, 24)
    fresh_hashes = np.array(next(c[2] for c in changes if c[0] == "insert"), np.uint32)
    queries.insert(len(ends) + 2, np.concatenate([fresh_hashes, rng.integers(0, 1 << 32, 90, dtype=np.uint64).astype(np.uint32)]))
    # (the deleted / re-inserted docs' OLD hashes lead their queries: the older segment's postings of them must be dropped)
    if form == "filtered":
        got = _check(fpx, p, queries, want_flags=64 | 256, not_flags=128)
    elif form == "two_parts":
        got = _check(fpx, p, queries, want_flags=64 | 128 | 256)
    else:
        ctx.set_option("query_wg", 0 if form == "packed" else 1)
        got = _check(fpx, p, queries, want_flags=4 if grouped else 0, not_flags=64 | 128)
    deleted = {ends[0], int(old[30])} | ({TOP} if form == "blocks" and wide else set())
    assert not any(r[0] in deleted for g in got for row in g for r in row), "a deleted doc came back"
    _found(got[0][len(ends):], live + [ends[1]])


# ---- f. narrow / wide records in the bins at their thresholds ----------------------------------------------------------------

@pytest.mark.parametrize("bq,B", [(1, 4096), (2, 8192), (3, 16384)])
def test_record_width_at_its_threshold(env, fresh, bq, B):
    """a group (binned path: k_probe_group drops records into bins of 2^bq queries, k_score_bin) whose declared max doc is
    (0xFFFFFFFF >> bq) - 1 (4-byte records) or 0xFFFFFFFF >> bq (8-byte ones), a doc AT that max hit by every query of the batch --
    every query-in-bin position.  The repeat stays on the device-sized path (nothing handed back), and rec32 0 / 1 give the same
    bytes as the oracle.  (Which width the bins took is not visible through the API: a host condition that wrongly allowed 4-byte
    records at the wide max is caught here -- the kernel refuses the record of the doc AT the max and the batch goes back to the general
    path --, one that wrongly refused them on the narrow side would only cost speed and is not.)"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(7600 + bq)
    ctx.set_option("query_wg", 0)
    o = fpx.SearchOptions(max_results=5, min_score=3, min_score_pct=10)
    for top in ((TOP >> bq) - 1, TOP >> bq):
        ctx.set_option("group_packed", 0)
        p = Pair(ctx)
        cols = [_span(top - 2 * 1500 + 1, 1500), _span(top - 1499, 1500)]
        raw = [_file(p, rng, cols[0], [int(cols[0][-1])], 1), _file(p, rng, cols[1], [top - 1, top], 2)]
        p.finish()
        assert all(g.grouped for g in p.gpu_segs) and p.gpu_segs[0].group_info()["packed"] == 0
        own = (_rows(raw[1], top) >> np.uint64(32)).astype(np.uint32)
        other = [(_rows(raw[i % 2], int(cols[i % 2][i % 1500])) >> np.uint64(32)).astype(np.uint32)[:4] for i in range(64)]
        queries = [np.concatenate([own[: 6 + i % 7], other[i % 64], rng.integers(0, 1 << 32, 6, dtype=np.uint64).astype(np.uint32)])
                   for i in range(B)]
        got = {}
        for rec32 in (1, 0):
            ctx.set_option("rec32", rec32)
            p.reader = fpx.IndexReader(fpx.Segments(ctx, p.gpu_segs))                 # (rec32_refused is sticky: a fresh snapshot)
            first, _ = p.reader.search_batch(queries, o)
            got[rec32], st = p.reader.search_batch(queries, o)
            # (the repeat on the device-sized path, binned by k_probe_group, scored by k_score_bin: a record the bins refused would
            # have sent the batch back to the general path)
            assert st.path_flags & (1 | 4 | 8) == 1 | 4 | 8, (hex(top), rec32, st.path_flags)
            assert got[rec32] == first
        assert got[1] == got[0]
        assert all(g and g[0][0] == top for g in got[1]), [g[:2] for g in got[1][:4]]
        p.check(queries, o, with_stats=False)                                       # (the oracle, on the snapshot of rec32 0)
        del p
        gc.collect()
