"""What the query-per-workgroup suites share (test_gpu_side_wg.py, test_gpu_words_wg.py, test_gpu_low_wg.py, test_gpu_low_wg_filtered.py,
test_gpu_hot_wg.py, test_gpu_wg_tail.py): the names of fpx_stats.path_flags' bits, the makers of items and queries, the handling of a
context's options, ONE World that files columns into a group and segments next to it, and both(): a batch under an option and under 0,
everything compared.  What differs between the suites is an argument here and a default in the suite's own few lines.

A helper module like fpx_testlib.py: no test, no fixture, and nothing but numpy at import (the library is loaded by open_context).

The makers draw from `rng` in a fixed order, with fixed shapes and dtypes: a world or a query of a given seed is the same bytes whichever
suite makes it, and test_wg_harness.py holds digests of them."""
import contextlib

import numpy as np

# fpx_stats.path_flags
SECOND_TRIP, GROUP, QUERY_WG, TWO_PARTS, FILTERED, SIDE, REDONE, WORDS, LOW = 2, 4, 64, 128, 256, 512, 1024, 2048, 4096
# the kernels' sizes (csrc/fpx_qsearch.hpp)
QS_MAX_HASHES, QS_REC_CAP, QS_TASKS_FILT = 4096, 8192, 512
# hashes of the low-floor suites' edge worlds: 1000 docs in each of eight columns, 1000 docs of column 0
HOT8, HOT1 = 0x4BCDEF01, 0x4CCDEF05
# the random hashes of the words suites' columns: noise below and above is out of every column's range
WORDS_LO, WORDS_HI = 0x10000000, 0xF0000000
U64 = np.uint64

STATS = ("scanned_blocks", "scanned_docs", "probes", "hits", "algorithmic_bytes")
_LABELS = ("blocks", "docs", "probes", "hits", "bytes")      # (as both() prints them)
FOUR, WITH_BYTES = 4, 5              # both(compare=...): the first four of STATS, or all of them


# ---- items and queries ----------------------------------------------------------------------------------------------------------

def post(hash_, ids):
    return (U64(hash_) << U64(32)) | np.asarray(ids, dtype=U64)


def rand_items(rng, ids, nh, extra=(), lo=0, hi=1 << 32):
    """the docs `ids` with `nh` random hashes in [lo, hi) each, and the postings (hash, docs) of `extra`"""
    docs = np.asarray(ids, dtype=U64)
    h = rng.integers(lo, hi, (len(docs), nh), dtype=U64)
    return np.unique(np.concatenate([((h << U64(32)) | docs[:, None]).ravel()] + [post(hh, d) for hh, d in extra]))


def rows(items, doc):
    return (items[(items & U64(0xFFFFFFFF)) == U64(doc)] >> U64(32)).astype(np.uint32)


def noise(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=U64).astype(np.uint32)


def aimed(rng, items, qlen, extra=(), lo=None, hi=None):
    """a query of `qlen` hashes: a random doc's of `items` (half the query at most), `extra`, the rest noise over the whole hash space
    (half of it inside [lo, hi) where given)"""
    doc = items[rng.integers(0, len(items))] & U64(0xFFFFFFFF)
    parts = [rows(items, doc)[:max(1, qlen // 2)], np.asarray(extra, dtype=np.uint32)]
    have = sum(len(x) for x in parts)
    if qlen > have:
        parts.append(noise(rng, qlen - have))
        if lo is not None:
            parts[-1][::2] = rng.integers(lo, hi, len(parts[-1][::2]), dtype=U64).astype(np.uint32)
    q = np.concatenate(parts)
    rng.shuffle(q)
    return q


def sampled(rng, items, n):
    """the hashes of `n` postings drawn from `items`: about n docs with a score of 1, a few with 2"""
    return (items[rng.choice(len(items), n, replace=False)] >> U64(32)).astype(np.uint32)


def usual(shared, double):
    """-> columns()' `extra`: `shared` a list of 2 / 3 / 4 / 70 docs, `double` a double in every column"""
    return lambda s, ids: [(shared, ids[: [2, 3, 4, 70][s % 4]]), (double, ids[:2])]


def exact(records, p, rng, head, singles, target):
    """a query of exactly `target` records by the suite's own count records(p, q): `head` (HOT8, HOT1 or neither), then hashes of one doc
    each (one of them may be some other doc's too), fifty of noise"""
    tail = noise(rng, 50)
    n = target - 1000 * 8 * (HOT8 in head) - 1000 * (HOT1 in head)
    for _ in range(6):
        q = np.concatenate([np.array(head, dtype=np.uint32), singles[:n], tail])
        r = records(p, q)
        if r == target:
            break
        n += target - r
    assert r == target and 0 < n <= len(singles), (r, target, n)
    rng.shuffle(q)
    return q


def legacy(fpx):
    """the legacy protocol's search (src/legacy.zig:192-197)"""
    return fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=10)


# ---- the context and its options ------------------------------------------------------------------------------------------------

def open_context():
    """-> (fpx, oracle, Pair, a context on device 0): what a suite's module-scoped `env` fixture yields"""
    from fpx_testlib import fpx, oracle, Pair
    return fpx, oracle, Pair, fpx.Context(0)


def reset(ctx, options):
    for name in options:
        ctx.set_option(name, -1)
    ctx.set_option("group_packed", -2)


@contextlib.contextmanager
def settings(env, monkeypatch, options, group_packed):
    """the body of a suite's per-test fixture: every file segment a direct-addressed candidate unless a test says otherwise, groups packed
    (1) or in directory + words form (0); `options` and group_packed reset before and afterwards"""
    ctx = env[3]
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    reset(ctx, options)
    ctx.set_option("group_packed", group_packed)
    try:
        yield env
    finally:
        reset(ctx, options)


# ---- a world --------------------------------------------------------------------------------------------------------------------

class World:
    """a Pair filled the way a live index grows: file segments that meet in ONE group, checkpoints in blocks (small decoded), merged
    segments that are direct-addressed alone, memory segments.

    packed: what group() asserts of the group's form (the suite's group_packed).  form: what file() takes a segment for when it is not
    told.  lo, hi: the range of columns()' random hashes.  snapshot_query_wg: the value of query_wg in force while a snapshot is made
    (2: a filtered group may be part 0 of a snapshot in two parts)"""

    def __init__(self, Pair, ctx, packed=1, form="column", lo=0, hi=1 << 32, snapshot_query_wg=None):
        self.p, self.ctx, self.items, self.index, self.commit = Pair(ctx), ctx, [], [], 1
        self.packed, self.form, self.lo, self.hi, self.snapshot_query_wg = packed, form, lo, hi, snapshot_query_wg

    def file(self, items, ids, alive=None, form="default", block_size=512):
        """form: "column" or "alone" (a direct-addressed candidate), "blocks", None (leave direct_min_items alone)"""
        if form == "default":
            form = self.form
        if form is not None:
            self.ctx.set_option("direct_min_items", (1 << 20) if form == "blocks" else 0)
        ids = np.asarray(ids, dtype=np.uint32)
        _, index = self.p.add_file(items, int(ids.min()), int(ids.max()), self.commit, ids, alive, block_size=block_size)
        self.items.append(items); self.index.append(index)
        self.commit += 1

    def columns(self, rng, cols, per, nh, extra=lambda s, ids: [], first=1, again=None, block_size=512, lo=None, hi=None):
        """`cols` columns of `per` docs x `nh` random hashes and extra(s, ids)'s postings, then group() -> the Pair, the first free doc.
        again: {doc of an older column: the hashes the NEWEST column writes it again with (None: its own, all of them)}"""
        lo, hi = self.lo if lo is None else lo, self.hi if hi is None else hi
        for s in range(cols):
            ids = np.arange(first + s * per, first + (s + 1) * per, dtype=np.int64)
            items = rand_items(rng, ids, nh, extra(s, ids), lo, hi)
            if s == cols - 1 and again:
                for d, hashes in again.items():
                    old = next(it for it in self.items if len(rows(it, d)))
                    items = np.unique(np.concatenate([items, post(0, [d]) | (np.asarray(rows(old, d) if hashes is None else hashes, dtype=U64) << U64(32))]))
                ids = np.array(sorted(list(ids) + list(again)), dtype=np.int64)
            self.file(items, ids, form="column", block_size=block_size)
        return self.group(cols), first + cols * per

    def group(self, cols):
        """the columns meet in a snapshot: one group of the suite's form"""
        if self.snapshot_query_wg is None:
            self.p.finish()
        else:
            self.finish()                                      # (the option around the snapshot; direct_min_items goes back with it)
        assert all(g.grouped for g in self.p.gpu_segs[:cols]), [g.layout_reason for g in self.p.gpu_segs]
        info = self.p.gpu_segs[0].group_info()
        assert info["packed"] == self.packed and info["columns"] == cols and info["line_columns"] == (8 if cols <= 8 else 16), info
        return self.p

    def memory(self, items, ids):
        ids = np.asarray(ids, dtype=np.uint32)
        self.p.add_memory(items, int(ids.min()), int(ids.max()), self.commit, ids)
        self.items.append(items)
        self.commit += 1

    def changes(self, changes):
        self.p.add_memory_changes(changes, self.commit)
        self.commit += 1

    def finish(self):
        self.ctx.set_option("direct_min_items", -1)
        if self.snapshot_query_wg is None:
            self.p.finish()
            return self.p
        self.ctx.set_option("query_wg", self.snapshot_query_wg)      # (the value in force when the snapshot is made)
        try:
            self.p.finish()
        finally:
            self.ctx.set_option("query_wg", -1)
        return self.p


# ---- a batch under an option and under 0 ----------------------------------------------------------------------------------------

def hist(ctx):
    h, unb = ctx.scan_histograms()
    return h.as_dict(), unb


def growth(a, b):
    return {k: ([y - x for x, y in zip(a[k], b[k])] if isinstance(a[k], list) else b[k] - a[k]) for k in a}


def figures(s):
    """a batch's statistics in the order of STATS"""
    return (s.scanned_blocks, s.scanned_docs, s.probes, s.hits, s.algorithmic_bytes)


def both(ctx, p, queries, opts, option, on, clear, want=0, want_not=0, also=(), compare=WITH_BYTES):
    """Pair.check under `option` = `on` with the path bits asserted (`want` set, `want_not` clear), then the batch under the option and
    under 0 (the bits `clear` clear), everything equal: results, the first `compare` of STATS -- also with Pair.check's --, per-query
    blocks / docs and the growth of the context's scan histograms (nothing unbucketed).  also: (option, value) pairs set around both runs
    and reset afterwards.  -> Pair.check's results and statistics"""
    try:
        for name, value in also:
            ctx.set_option(name, value)
        ctx.set_option(option, on)
        got, st = p.check(queries, opts)
        print(f"{option} {on}: path_flags {st.path_flags}, {' / '.join(_LABELS[:compare])} {figures(st)[:compare]}")
        assert st.path_flags & want == want and not st.path_flags & want_not, (st.path_flags, want, want_not)
        h0, _ = hist(ctx)                                      # (the order of the searches and the snapshots: growth() compares like with like)
        g1, s1, qb1, qd1 = p.reader.search_batch_stats(queries, opts)
        h1, unb1 = hist(ctx)
        ctx.set_option(option, 0)
        g0, s0, qb0, qd0 = p.reader.search_batch_stats(queries, opts)
        h2, unb2 = hist(ctx)
    finally:
        ctx.set_option(option, -1)
        for name, _ in also:
            ctx.set_option(name, -1)
    f1, f0, ft = figures(s1)[:compare], figures(s0)[:compare], figures(st)[:compare]
    print(f"{option} 0: path_flags {s0.path_flags}, {f0}; {option} {on} again: {s1.path_flags}, {f1}")
    assert not s0.path_flags & clear, (s0.path_flags, clear)
    assert s1.path_flags & want == want and not s1.path_flags & want_not, (s1.path_flags, want, want_not)
    assert g1 == got and g0 == got
    assert f1 == f0, (f1, f0)
    assert f1 == ft, (f1, ft)
    assert [int(x) for x in qb1] == [int(x) for x in qb0] and [int(x) for x in qd1] == [int(x) for x in qd0]
    assert growth(h0, h1) == growth(h1, h2), (growth(h0, h1), growth(h1, h2))
    assert unb1 == 0 and unb2 == 0, (unb1, unb2)
    return got, st

