"""k_search_classes (csrc/fpx_qsearch.hpp, option hot_wg = 1): a query whose hit records outgrow the 8192 slots of k_search_query's LDS
array -- a dozen hot hashes of 1000+ docs -- no longer sends the whole batch to the pipeline and the next 32 batches after it: the first
pass names it in the batch's redo list and counts nothing for it, and k_search_classes searches it once per DOC CLASS, keeping one class
of records each time.  fpx_stats.path_flags bit 10 (1024) says that some queries of the batch were redone that way.

Every case goes through Pair.check under hot_wg = 1 (results and every query's scanned blocks / docs == the oracle's) and is then run
again under hot_wg = 1 and 0 and compared byte for byte: results, scanned_blocks, scanned_docs, probes, hits, per-query blocks / docs and
the growth of the context's scan histograms.  Under hot_wg = 0 the same batch is handed back (bit 64 clear) and the snapshot backs off;
the helper drains that back-off before it returns.

Kernel mutations this file was seen to catch, each built as a library of its own and run against the file on an MI355X (the runs are in
profiles/r11_hot_wg.txt; "all heavy cases" = every case but the superseded-doc one, which never reaches k_search_classes):

* the class test dropped at one emission site: the rounds' inline words (kept = keep) -- all heavy cases fail; the wave-walked lists
  (emit1 without the test) -- all heavy cases; the tasks' words and list heads (km not masked) -- all heavy cases; the memory segments'
  table -- test_memory_segments_next_to_the_group alone, as it should be;
* statistics added in every pass (q_stats true, the wave totals added in every pass) -- all heavy cases: blocks, docs and probes are C
  times the oracle's;
* s_ccnt reset between passes -- every case whose redone query has candidates in more than one class (one_heavy_query, the 1000-doc list,
  memory segments, candidates_across_the_classes, three_heavy_queries, more_heavy_queries_than_the_limit);
* first-pass statistics not withheld for a query that goes to the redo list -- all heavy cases (counted twice);
* C sized without the factor of 2 -- test_the_boundary_and_the_sizing_of_the_classes (exactly 2 x 8192 records: two classes, one
  overflows, a hand-back) and the 32-class query of test_a_query_of_more_than_32_classes (16 classes of 8192 on average overflow)."""
import numpy as np
import pytest

import wg_harness as wg
from wg_harness import FILTERED, QS_REC_CAP, QUERY_WG, REDONE, SECOND_TRIP, U64, figures as _figures, growth as _growth, hist as _hist, post as _post

pytestmark = pytest.mark.gpu

HOT, SHARED, CROWD, SINGLE = 0x12345678, 0x0BADF00D, 0x51515151, 0x70000000
OPTIONS = ("hot_wg", "query_wg")


@pytest.fixture(scope="module")
def env():
    e = wg.open_context()
    yield e
    wg.reset(e[3], OPTIONS)


@pytest.fixture
def hot(env, monkeypatch):
    """every file segment a direct-addressed candidate, groups packed; the options reset afterwards"""
    with wg.settings(env, monkeypatch, OPTIONS, group_packed=1) as e:
        yield e


class World:
    """`nseg` file segments of `per` docs x 48 random hashes in one packed group; `nhot` hot hashes of `hot_docs` docs each, dealt to the
    segments in turn (all_segs: every one of them in every segment); in segment 0 `singles` hashes of one doc each and a crowd of docs
    that share thirty hashes, in segment 1 the 3000-doc HOT hash; then what `memory(world, first free doc)` adds"""

    def __init__(self, Pair, ctx, seed, nseg=3, per=4000, nhot=12, hot_docs=1500, all_segs=False, singles=0, crowd=0, big=False, first=1, memory=None):
        rng = np.random.default_rng(seed)
        self.rng, self.p, self.items = rng, Pair(ctx), []
        self.hots = [0x40000000 + 977 * k for k in range(nhot)]
        self.singles = [SINGLE + 7919 * k for k in range(singles)]
        for s in range(nseg):
            f = first + s * per
            docs = np.arange(f, f + per, dtype=U64)
            h = rng.integers(0, 1 << 32, (per, 48), dtype=U64)
            items = [((h << U64(32)) | docs[:, None]).ravel(), _post(SHARED, docs[: [2, 3, 4, 70][s % 4]])]
            for k in (self.hots if all_segs else self.hots[s::nseg]):
                items.append(_post(k, docs[:hot_docs]))
            if s == 0:
                items += [_post(k, docs[2000 + i: 2001 + i]) for i, k in enumerate(self.singles)]
                items += [_post(CROWD + k * 7919, docs[100:100 + crowd]) for k in range(30 if crowd else 0)]
            if s == 1 and big:
                items.append(_post(HOT, docs[:3000]))
            items = np.unique(np.concatenate(items))
            self.p.add_file(items, f, f + per - 1, s + 1, np.arange(f, f + per, dtype=np.uint32))
            self.items.append(items)
        if memory is not None:
            memory(self, first + nseg * per, nseg + 1)
        self.p.finish()
        assert all(g.grouped for g in self.p.gpu_segs[:nseg]), [g.layout_reason for g in self.p.gpu_segs]

    def plain(self, i, qlen=1000, aimed=True):
        src = self.items[i % len(self.items)]
        doc = src[self.rng.integers(0, len(src))] & U64(0xFFFFFFFF)
        own = (src[(src & U64(0xFFFFFFFF)) == doc] >> U64(32)).astype(np.uint32)[:max(1, qlen // 2) if aimed else 0]
        own = own[~np.isin(own, np.array(self.hots + self.singles + [HOT], dtype=np.uint32))]
        q = np.concatenate([own, np.array([SHARED, SHARED], dtype=np.uint32), self.rng.integers(0, 1 << 32, qlen - len(own) - 2, dtype=U64).astype(np.uint32)])
        self.rng.shuffle(q)
        return q

    def heavy(self, i, extra=(), nhot=None, qlen=900, aimed=True):
        q = np.concatenate([self.plain(i, qlen, aimed), np.array(self.hots[:nhot], dtype=np.uint32), np.asarray(extra, dtype=np.uint32)])
        self.rng.shuffle(q)
        return q

    def records(self, q):
        """a query's hit records, as the reference counts them (a hash's docs beyond what FileSegment.search returns are none)"""
        return self.p.osnap.search(q, 40, None, 10, with_stats=True)[1].scanned_docs


def _drain(p, plain):
    """batches until the snapshot's back-off after a hand-back is over"""
    for _ in range(40):
        if p.reader.search_batch(plain, p.http)[1].path_flags & QUERY_WG:
            return
    raise AssertionError("the query-per-workgroup path did not come back")


def _both(fpx, ctx, w, queries, opts, plain, redone=True, want=0):
    """Pair.check under hot_wg = 1 with the path bits asserted, then the batch under hot_wg = 1 and 0, everything equal.  Not the harness's
    both(): between the two runs a plain batch shows that nothing backed off, so the histograms are read once more (h1b) before the run
    under 0, and a handed-back batch's back-off is drained at the end"""
    p = w.p
    p.http = fpx.http_options()
    want1 = QUERY_WG | (REDONE if redone else 0) | want
    try:
        ctx.set_option("hot_wg", 1)
        got, st = p.check(queries, opts)
        assert st.path_flags & want1 == want1 and (redone or not st.path_flags & REDONE), (st.path_flags, want1)
        h0, _ = _hist(ctx)
        g1, s1, qb1, qd1 = p.reader.search_batch_stats(queries, opts)
        h1, unb1 = _hist(ctx)
        assert s1.path_flags & want1 == want1, (s1.path_flags, want1)
        # no back-off: the very next plain batch is on the path, and nothing of it is redone
        _, sn = p.reader.search_batch(plain, p.http)
        assert sn.path_flags & QUERY_WG and not sn.path_flags & REDONE, sn.path_flags
        ctx.set_option("hot_wg", 0)
        h1b, _ = _hist(ctx)
        g0, s0, qb0, qd0 = p.reader.search_batch_stats(queries, opts)
        h2, unb2 = _hist(ctx)
        assert not s0.path_flags & REDONE, s0.path_flags
        assert bool(s0.path_flags & QUERY_WG) == (not redone), s0.path_flags        # (a heavy batch: handed back, as before)
        if redone:
            _drain(p, plain)
    finally:
        ctx.set_option("hot_wg", -1)
    assert g1 == got and g0 == got
    t1, t0 = _figures(s1)[:wg.FOUR], _figures(s0)[:wg.FOUR]      # (blocks, docs, probes and hits: this suite never compared algorithmic_bytes)
    assert t1 == t0, (t1, t0)
    assert t1 == _figures(st)[:wg.FOUR]
    assert [int(x) for x in qb1] == [int(x) for x in qb0] and [int(x) for x in qd1] == [int(x) for x in qd0]
    assert _growth(h0, h1) == _growth(h1b, h2), (_growth(h0, h1), _growth(h1b, h2))
    assert unb1 == 0 and unb2 == 0, (unb1, unb2)
    return got, st, s1


def _option_sets(fpx):
    return [fpx.http_options(), fpx.SearchOptions(max_results=100, min_score=3, min_score_pct=0)]


@pytest.mark.parametrize("nseg", [3, 16])
def test_one_heavy_query_among_fifteen_plain_ones(hot, nseg):
    """lines of 8 hash values (3 columns) and of 4 (16 columns); a floor of 3 makes every hot doc a candidate: thousands, over the classes"""
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 99 + nseg, nseg=nseg, per=4000 if nseg == 3 else 1600)
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[5] = w.heavy(5)
    assert w.records(heavy[5]) > QS_REC_CAP
    for opts in _option_sets(fpx):
        got, st, s1 = _both(fpx, ctx, w, heavy, opts, plain)
    if nseg == 3:                                        # (four hot hashes on the same 1500 docs of a segment: every one of them reaches 3)
        assert st.path_flags & SECOND_TRIP and len(got[5]) == 100
    # the option is off by default: the heavy batch is handed back
    _, st_d = w.p.reader.search_batch(heavy, fpx.http_options())
    assert not st_d.path_flags & (QUERY_WG | REDONE)


def _trimmed(w, i, target):
    """a query of exactly `target` records: as many hot hashes as fit, then hashes of one doc each"""
    for nhot in range(len(w.hots), -1, -1):
        base = w.heavy(i, nhot=nhot)
        r = w.records(base)
        if r <= target:
            break
    need = target - r
    assert 0 <= need <= len(w.singles), (r, target, len(w.singles))
    q = np.concatenate([base, np.array(w.singles[:need], dtype=np.uint32)])
    w.rng.shuffle(q)
    assert w.records(q) == target
    return q


def test_the_boundary_and_the_sizing_of_the_classes(hot):
    """exactly QS_REC_CAP records: the array takes them, nothing is redone; one more: redone.  Exactly 2 x QS_REC_CAP: four classes of
    4096 on average -- two classes of 8192 on average would overflow again"""
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 7, nhot=18, singles=1600)
    plain = [w.plain(i) for i in range(16)]
    full, over, twice = _trimmed(w, 3, QS_REC_CAP), _trimmed(w, 3, QS_REC_CAP + 1), _trimmed(w, 4, 2 * QS_REC_CAP)
    for q, redone in ((full, False), (over, True), (twice, True)):
        batch = list(plain)
        batch[11] = q
        _, st, s1 = _both(fpx, ctx, w, batch, fpx.http_options(), plain, redone=redone)
        assert s1.hits == sum(w.records(x) for x in batch)


def test_a_list_of_more_than_1000_docs_walked_by_the_wave(hot):
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 11, big=True)
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[0] = w.heavy(0, extra=[HOT, 0, 0xFFFFFFFF, HOT])
    heavy[15] = w.heavy(15, extra=[HOT])
    for opts in _option_sets(fpx):
        _both(fpx, ctx, w, heavy, opts, plain)


def test_memory_segments_next_to_the_group(hot):
    """the hot hashes are in the group AND in the memory segments' table; a memory doc lies below the group's first doc (its record is
    doc - gmin modulo 2^32: the class is taken from that value at every site)"""
    fpx, oracle, Pair, ctx = hot

    def memory(w, nxt, commit):
        for m in range(3):
            ids = [5 + m] + list(range(nxt + m * 60, nxt + m * 60 + 60))
            docs = np.array(ids, dtype=U64)
            h = w.rng.integers(0, 1 << 32, (len(ids), 48), dtype=U64)
            items = [((h << U64(32)) | docs[:, None]).ravel(), _post(SHARED, docs[:3])] + [_post(k, docs) for k in w.hots]
            items = np.unique(np.concatenate(items))
            w.p.add_memory(items, min(ids), max(ids), commit + m, np.array(ids, dtype=np.uint32))
            w.items.append(items)

    w = World(Pair, ctx, 13, first=1001, memory=memory)
    plain = [w.plain(i) for i in range(16)]              # (every other query aims at a doc of a memory segment)
    heavy = list(plain)
    heavy[6] = w.heavy(6)
    heavy[9] = w.heavy(5)
    opts = fpx.SearchOptions(max_results=500, min_score=10, min_score_pct=0)      # (a memory doc holds all twelve hot hashes: 183 candidates of them)
    for o in (fpx.http_options(), opts):
        got, st, s1 = _both(fpx, ctx, w, heavy, o, plain)
    found = {d for d, s in got[6]}
    assert {5, 6, 7} <= found and len([d for d in found if d > 13000]) == 180, sorted(found)[:8]


def test_candidates_across_the_classes(hot):
    """250 docs share thirty hashes and sit under four hot hashes: 250 candidates at a floor of 25 -- more than the query's four slots,
    than the 32 of its LDS buffer, than the exact table's 192 --, found class by class"""
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 17, crowd=250)
    crowd = [CROWD + k * 7919 for k in range(30)]
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[2] = w.heavy(2, extra=crowd, aimed=False)          # (noise, the hot hashes and the crowd's: nothing above the crowd)
    heavy[8] = w.heavy(8, extra=crowd[:27], aimed=False)
    for opts in (fpx.SearchOptions(max_results=500, min_score=25, min_score_pct=0), fpx.SearchOptions(max_results=10, min_score=28, min_score_pct=95)):
        got, st, s1 = _both(fpx, ctx, w, heavy, opts, plain, want=SECOND_TRIP)
    assert len(got[2]) == 10 and len(got[8]) == 10
    got, _, _ = _both(fpx, ctx, w, heavy, fpx.SearchOptions(max_results=500, min_score=25, min_score_pct=0), plain, want=SECOND_TRIP)
    assert len(got[2]) == 250 and len(got[8]) == 250


def test_three_heavy_queries_two_of_them_identical_and_the_batch_resident(hot):
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 19)
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[2] = w.heavy(2)
    heavy[9] = heavy[2].copy()
    heavy[13] = w.heavy(13, nhot=9)
    for opts in _option_sets(fpx):
        got, st, s1 = _both(fpx, ctx, w, heavy, opts, plain)          # (from host memory, and through fpx_search_batch_stats)
        assert got[2] == got[9]
        ctx.set_option("hot_wg", 1)
        try:
            qb = fpx.QueryBatch(ctx, queries=heavy, options=opts)
            o, n, st_r = fpx.search_resident(w.p.reader, qb)
            qb.release()
        finally:
            ctx.set_option("hot_wg", -1)
        assert st_r.path_flags & (QUERY_WG | REDONE) == QUERY_WG | REDONE, st_r.path_flags
        assert fpx.results_to_lists(o, n) == got
        assert (st_r.scanned_blocks, st_r.scanned_docs, st_r.probes, st_r.hits) == (s1.scanned_blocks, s1.scanned_docs, s1.probes, s1.hits)


def _handed_back(fpx, ctx, w, heavy, plain):
    """under hot_wg = 1 the batch goes to the pipeline as before: == the oracle, bit 1024 clear, and the next 32 batches stay there"""
    http = fpx.http_options()
    ctx.set_option("hot_wg", 1)
    try:
        _, st_p = w.p.reader.search_batch(plain, http)
        assert st_p.path_flags & QUERY_WG, st_p.path_flags
        got, st = w.p.reader.search_batch(heavy, http)
        assert not st.path_flags & (QUERY_WG | REDONE), st.path_flags
        for q, g in zip(heavy, got):
            assert g == w.p.osnap.search(q, 40, None, 10)
        flags = [w.p.reader.search_batch(plain, http)[1].path_flags & (QUERY_WG | REDONE) for _ in range(34)]
    finally:
        ctx.set_option("hot_wg", -1)
    assert flags == [0] * 32 + [QUERY_WG] * 2, flags


def test_more_heavy_queries_than_the_limit_go_back_to_the_pipeline(hot):
    """a batch of 16: up to four queries are redone, five are a hot batch"""
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 23)
    plain = [w.plain(i) for i in range(16)]
    four, five = list(plain), list(plain)
    for i in (1, 4, 7, 10):
        four[i] = five[i] = w.heavy(i)
    five[14] = w.heavy(14)
    _both(fpx, ctx, w, four, fpx.http_options(), plain)
    _handed_back(fpx, ctx, w, five, plain)


def test_a_query_of_more_than_32_classes_goes_back_to_the_pipeline(hot):
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 29, nhot=48, all_segs=True)
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[7] = w.heavy(7)
    assert w.records(heavy[7]) > 32 * (QS_REC_CAP // 2), w.records(heavy[7])
    _handed_back(fpx, ctx, w, heavy, plain)
    # ... and 32 classes are taken: thirty hashes in all three segments
    few = list(plain)
    few[7] = w.heavy(7, nhot=30)
    assert 16 * (QS_REC_CAP // 2) < w.records(few[7]) <= 32 * (QS_REC_CAP // 2), w.records(few[7])
    _both(fpx, ctx, w, few, fpx.http_options(), plain)


def test_a_group_with_a_superseded_doc_keeps_the_hand_back(hot):
    """query_wg = 2 takes the filtered instantiation, which has no redo list"""
    fpx, oracle, Pair, ctx = hot

    def memory(w, nxt, commit):                       # doc 17 of the first file segment, written again
        ids = [17] + list(range(nxt, nxt + 60))
        docs = np.array(ids, dtype=U64)
        h = w.rng.integers(0, 1 << 32, (len(ids), 48), dtype=U64)
        items = np.unique(((h << U64(32)) | docs[:, None]).ravel())
        w.p.add_memory(items, min(ids), max(ids), commit, np.array(ids, dtype=np.uint32))
        w.items.append(items)

    w = World(Pair, ctx, 31, memory=memory)
    plain = [w.plain(i) for i in range(16)]
    heavy = list(plain)
    heavy[5] = w.heavy(5)
    ctx.set_option("query_wg", 2)
    try:
        _, st = w.p.reader.search_batch(plain, fpx.http_options())
        assert st.path_flags & FILTERED, st.path_flags
        _handed_back(fpx, ctx, w, heavy, plain)
    finally:
        ctx.set_option("query_wg", -1)


def test_a_deadline_that_has_passed_is_a_timeout_and_no_partial_results(hot):
    """25 200 queries of 1000 hashes from host memory, one in fifteen heavy, against a deadline of 1 ms: the 100 MB of hashes alone need
    longer than that on the link, so the deadline HAS passed when the call first waits -- error.SearchTimeout, no results, and the same
    call without a deadline afterwards is complete and correct (nothing of the cancelled batch is left in the workspace)"""
    fpx, oracle, Pair, ctx = hot
    w = World(Pair, ctx, 37)
    distinct = [w.heavy(i) if i % 15 == 0 else w.plain(i) for i in range(600)]
    queries = distinct * 42
    ctx.set_option("hot_wg", 1)
    try:
        want, st = w.p.reader.search_batch(queries, fpx.http_options())
        assert st.path_flags & (QUERY_WG | REDONE) == QUERY_WG | REDONE, st.path_flags
        with pytest.raises(fpx.SearchTimeout) as e:
            w.p.reader.search_batch(queries, fpx.http_options(), timeout_ms=1)
        assert e.value.status == -2
        again, st2 = w.p.reader.search_batch(queries, fpx.http_options())
        assert again == want and st2.path_flags & (QUERY_WG | REDONE) == QUERY_WG | REDONE
    finally:
        ctx.set_option("hot_wg", -1)
    assert want[600:1200] == want[:600]
    for i in (0, 1, 15, 599):
        assert want[i] == w.p.osnap.search(queries[i], 40, None, 10), i
