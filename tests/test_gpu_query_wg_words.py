"""The slot arithmetic of k_search_query (csrc/fpx_qsearch.hpp): how a lane classifies the words of its hash (docs, second words of
doubles, gap positions, list references), where it stores the docs among them in the query's record array, what it leaves to the tasks
(words beyond its own twelve, words that overflowed the line into `ext`, lists), and where `gmin` -- the one base the words of a packed
group count from -- is added back.  Against the oracle through Pair.check: results and every query's scanned blocks / docs; every batch
asserts path_flags & 64 (a query per workgroup).

The data is made for it.  A CASE is a hash T present in k columns, d of them holding two docs (a double: two words), in a line of
its own; the hashes before it in the same line hold n0 words, so that T's words start at n0 (`start`): the cases cross the lane's
16-byte pieces (4, 8, 12 words), the task size (8 more) and the end of the line (28 / 29 words inline, the rest in `ext`) at every
words count k + d from 0 to 2 x columns.  LIST cases put a column of three to five docs (a list reference) at every word position: among
the lane's own words, in a words task and in `ext`.  The docs come from a small pool per column, so that they reach the floor.

* groups of 16 columns (lines of four hash values) and of 8 (lines of eight);
* a group whose gmin is above 2^31 next to memory segments whose docs lie BELOW gmin (the records are doc - gmin modulo 2^32);
* the same cases through query_wg = 2 with one dead doc of the pool per column (the filtered form tests the absolute doc).

Deliberate mutations of the kernel that these tests were seen to catch: a slot with no doc below it stored onto the lane's first doc
instead of the sink, one word beyond the lane's own classified, a words task's count off by one, gmin not added at hand-over (every
test); a memory segment's record left absolute (the gmin tests); the dead test given the relative doc (the filtered tests)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = 0x20000000             # the cases' lines start here, 64 hash values apart
POOL = 6                      # docs per column that the cases draw from


@pytest.fixture(scope="module")
def env():
    from fpx_testlib import fpx, oracle, Pair
    ctx = fpx.Context(0)
    yield fpx, oracle, Pair, ctx
    ctx.set_option("query_wg", -1)
    ctx.set_option("group_packed", -2)


def _cases(ncol):
    """(k, d, n0, list position or None): T in k columns, the first d (rotated) doubles, n0 words of the neighbour before them"""
    out = []
    for w in range(0, 2 * ncol + 1):
        ds = {max(0, w - ncol), w // 2, (max(0, w - ncol) + w // 2) // 2}          # fewest doubles, most, between
        for d in sorted(ds):
            k = w - d
            if k > ncol or d > k:
                continue
            for n0 in (0, 3, 7, 11, 19, 23, 27):
                out.append((k, d, n0, None))
    for lp in range(ncol):                                                           # a list in column position lp of all ncol
        for d in (0, min(lp, 6)):                                                    # (doubles before it move its word up)
            for n0 in (0, 9, 17, 25):
                out.append((ncol, d, n0, lp))
    return out


def _world(fpx, Pair, ctx, monkeypatch, ncol, first_doc=1, per=600, memory_below=False, dead=False, seed=77):
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    ctx.set_option("group_packed", 1)
    rng = np.random.default_rng(seed + ncol)
    cases = _cases(ncol)
    firsts = [first_doc + s * per for s in range(ncol)]
    posts = [[] for _ in range(ncol)]

    def post(s, h, docs):
        posts[s].append((np.uint64(h) << np.uint64(32)) | np.asarray(docs, dtype=np.uint64))

    def words(h, c, k, d, lp=None):
        """hash h in k columns (rotated by c), d doubles; column position lp a list of 3 .. 5 docs"""
        cols = sorted((c + i) % ncol for i in range(k))
        dbl = set(cols[(c + i) % k] for i in range(d)) if lp is None else set(cols[:d]) - {cols[lp]}
        for i, s in enumerate(cols):
            pool = firsts[s] + 10 + (np.arange(POOL) + c) % POOL
            n = (3 + c % 3) if (lp is not None and i == lp) else (2 if s in dbl else 1)
            post(s, h, pool[:n])

    targets = []
    for c, (k, d, n0, lp) in enumerate(cases):
        # T is the line's fourth hash (at 16 columns: beyond the double flags) or, at 16 columns, its second; the n0 words before it belong
        # to the line's first hash and, beyond 2 x columns of them, its third
        t = BASE + c * 64 + (3 if ncol == 8 or c % 4 == 3 else 1)
        words(t, c, k, d, lp)
        for off, n in ((0, min(n0, 2 * ncol)), (2, n0 - min(n0, 2 * ncol))):
            if n:
                words(BASE + c * 64 + off, c + 1, min(n, ncol), max(0, n - ncol))
        targets.append(t)
    p = Pair(ctx)
    allitems = []
    for s in range(ncol):
        docs = np.arange(firsts[s], firsts[s] + per, dtype=np.uint64)
        h = rng.integers(0, 1 << 32, (per, 24), dtype=np.uint64)
        items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel()] + posts[s]))
        p.add_file(items, firsts[s], firsts[s] + per - 1, s + 1, np.arange(firsts[s], firsts[s] + per, dtype=np.uint32))
        allitems.append(items)
    commit = ncol + 1
    if memory_below:
        # memory segments whose docs lie below the group's gmin: they share case hashes with the pool (and score with it)
        for m in range(2):
            docs = np.arange(1000 + 100 * m, 1000 + 100 * m + 40, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (40, 24), dtype=np.uint64)
            extra = [(np.uint64(t) << np.uint64(32)) | docs[:3] for t in targets[m::5]]
            items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel()] + extra))
            p.add_memory(items, int(docs[0]), int(docs[-1]), commit, docs.astype(np.uint32))
            allitems.append(items)
            commit += 1
    if dead:
        # one doc of every column's pool written again, with other hashes, in a memory segment: superseded in its column
        gone = [firsts[s] + 10 + s % POOL for s in range(ncol)]
        nxt = first_doc + ncol * per
        ids = sorted(gone + list(range(nxt, nxt + 20)))
        h = rng.integers(0, 1 << 32, (len(ids), 24), dtype=np.uint64)
        items = np.unique(((h << np.uint64(32)) | np.asarray(ids, dtype=np.uint64)[:, None]).ravel())
        p.add_memory(items, ids[0], ids[-1], commit, np.asarray(ids, dtype=np.uint32))
        allitems.append(items)
    p.finish()
    ctx.set_option("group_packed", -2)
    assert all(g.direct and g.grouped for g in p.gpu_segs[:ncol]), [g.layout_reason for g in p.gpu_segs[:ncol]]
    return p, cases, np.asarray(targets, dtype=np.uint32), rng


def _queries(rng, targets, with_neighbours=True):
    """every case's hash in some query: slices of 50 cases (shuffled) among noise -- two rounds, the second partial --, every third slice
    with the line's first hash as well, and one query of a fifth of them"""
    qs = []
    order = rng.permutation(len(targets))
    for i in range(0, len(order), 50):
        t = targets[order[i:i + 50]]
        parts = [t, rng.integers(0, 1 << 32, 250, dtype=np.uint64).astype(np.uint32)]
        if with_neighbours and (i // 50) % 3 == 0:
            parts.append((t & ~np.uint32(63)))
        q = np.concatenate(parts)
        rng.shuffle(q)
        qs.append(q)
    # (a fifth of them: a query's records have to fit its workgroup's array of 8192)
    q = np.concatenate([targets[::5], targets[::10] & ~np.uint32(63), rng.integers(0, 1 << 32, 600, dtype=np.uint64).astype(np.uint32)])
    rng.shuffle(q)
    qs.append(q)
    return qs


def _options(fpx):
    return [fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0), fpx.SearchOptions(max_results=40, min_score=8, min_score_pct=10)]


@pytest.mark.parametrize("ncol", [16, 8])
def test_words_of_a_hash_at_every_count_and_start(env, ncol, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, cases, targets, rng = _world(fpx, Pair, ctx, monkeypatch, ncol)
    assert {k + d for k, d, _, lp in cases if lp is None} == set(range(2 * ncol + 1))
    queries = _queries(rng, targets)
    for opts in _options(fpx):
        got, st = p.check(queries, opts)
        assert st.path_flags & 64, f"the batch did not run k_search_query ({st.path_flags})"
    assert any(len(g) > 1 for g in got)
    # one case per query: a failure names the case
    singles = [np.concatenate([targets[c:c + 1], targets[(c + 1) % len(targets)::97][:8], rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)])
               for c in range(len(targets))]
    got, st = p.check(singles, fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0))
    assert st.path_flags & 64


@pytest.mark.parametrize("ncol", [16, 8])
def test_gmin_above_2_31_with_memory_docs_below_it(env, ncol, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, cases, targets, rng = _world(fpx, Pair, ctx, monkeypatch, ncol, first_doc=0x90000000, memory_below=True)
    queries = _queries(rng, targets)
    for opts in _options(fpx):
        got, st = p.check(queries, opts)
        assert st.path_flags & 64, f"the batch did not run k_search_query ({st.path_flags})"
    ids = [r[0] for g in got for r in g]
    assert any(i >= 0x90000000 for i in ids) and any(i < 2000 for i in ids), "the queries reach docs on both sides of gmin"


@pytest.mark.parametrize("ncol,first_doc", [(16, 1), (8, 0x90000000)])
def test_filtered_form_with_a_dead_doc_in_every_column(env, ncol, first_doc, monkeypatch):
    fpx, oracle, Pair, ctx = env
    p, cases, targets, rng = _world(fpx, Pair, ctx, monkeypatch, ncol, first_doc=first_doc, dead=True)
    queries = _queries(rng, targets)
    gone = {first_doc + s * 600 + 10 + s % POOL for s in range(ncol)}
    ctx.set_option("query_wg", 2)
    try:
        for opts in _options(fpx):
            got, st = p.check(queries, opts)
            assert st.path_flags & 64, f"the batch did not run k_search_query ({st.path_flags})"
            assert st.path_flags & 256, f"not the filtered form ({st.path_flags})"
            assert not gone & {r[0] for g in got for r in g}, "a superseded doc was returned"
    finally:
        ctx.set_option("query_wg", -1)
