"""The unfiltered rounds of k_search_query and k_search_classes (csrc/fpx_qsearch.hpp, round_coop): what is per HASH is made once, by the
hash's own lane, and goes to the eight lanes of its group ready-made --

* the RANGE WORD: bit w set = word w of the hash's line (position w - 3) is one of the hash's inline words, and the SECOND-WORD WORD: bit
  w set = it is the second word of a double; a lane's share of line k is nibble `sub` of each;
* the line's NUMBER in the group (0 for a hash that is no probe), from which a load is one shift and one add.

Against the oracle through Pair.check: results and every query's scanned blocks / docs (a wrong bit of the second-word word moves nothing
but a query's scanned blocks); every batch asserts path_flags & 64.  One small world per column count, lines of their own 64 hash values
apart whose hashes hold a given sequence of words:

* the range word: a line for every start 0 .. 32 and the lengths 1 .. 5, up to exactly the inline limit (29 words in the line), one over
  it (28 and the offset in word 31), 2 x columns, and a hash that ends at the limit of a line with more words behind it: every position
  of a range's two ends in a lane's four words, ranges inside one lane and across two to eight, ranges ending at word 31 and cut at 28;
* the second-word word: at starts 0, 1, 2, 3, 4, 27, 28 no double, all doubles, a double at the first column only, at the last only,
  alternating;
* lists: a group of lanes whose eight lines each hold a list reference -- in eight different lanes' registers, and all in ONE lane's --;
  two and three list references in one lane, of one line and of different lines of the group; a gap mark before two lists in one lane
  (the gap positions are looked up in the column's block index and confirmed by the oracle), at every alignment; a list reference as a
  hash's last inline word (word 31, and word 30 of a line of 28) and one in `ext`;
* addresses: lines in the LAST chunk of the hash space (0xFFFFFFF0 .. 0xFFFFFFFE) and in the first, probed in one query; a query in which
  every hash that one load instruction reads for is a duplicate but one; a query of length 1; lengths 255 / 256 / 257;
* the same lines next to a memory segment (the MEM instantiations) and in a query that outgrows the record array and is redone in doc
  classes under hot_wg = 1 (k_search_classes shares the rounds).

Deliberate mutations of the kernel, each built as a library of its own and run against this file (the runs are in
profiles/r14_ab_k_search_query.txt): the range word shifted up by one word; the second-word word shifted by one; the nibble taken at
4 (sub ^ 1) by lanes 2 .. 7; a lane's second list dropped.  (The first and the third in forms that never hand a line's HEAD words to
the walk: a head word with bit 31 set would be followed as a list reference to an address that no list is at.)  Two mutations that the
round's issue named change no result by construction and were not run: the second-word word not cut to the range word (it is only ever
looked at under the kept words, which are: the kernel does not cut it) and a non-probe's line number left at its hash's (such a lane has
an empty range word: it classifies nothing of what it read -- only the memory-side request count sees it)."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = 0x30000000             # the made lines start here, 64 hash values apart
TOP = (0xFFFFFFF0, 0xFFFFFFF1, 0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE)      # made hashes of the last lines of the hash space
LOW = 0                       # the group's first line (what a lane without a probe reads)
HOTS = 0x50000000             # hot hashes: a list of HOT_DOCS docs in every column
HOT_DOCS = 200
POOL = 8                      # docs per column that the made hashes draw from
GAP_COL = 4                   # the column whose block boundaries give the gap positions
REC_CAP = 8192                # csrc/fpx_qsearch.hpp: QS_REC_CAP
QUERY_WG, FILTERED, REDONE = 64, 256, 1024
S, D, LST = 1, 2, 3           # a column's words: one doc, a double (two words), a list reference
STARTS_SECOND = (0, 1, 2, 3, 4, 27, 28)
PATTERNS = {"none": [S] * 6, "all": [D] * 6, "first": [D] + [S] * 5, "last": [S] * 5 + [D], "alt": [D, S] * 3}


def _kinds(t, maxcols):
    """a hash of t words in as few doubles as its columns allow"""
    k = min(t, maxcols)
    assert t - k <= k
    return [D] * (t - k) + [S] * (2 * k - t)


def _filler(s, ncol):
    """hashes whose words add up to s: what lies before a hash that starts at s"""
    out = []
    while s > 0:
        t = min(s, 2 * ncol)
        out.append(_kinds(t, ncol))
        s -= t
    return out


def _range_lengths(start, ncol):
    return sorted(L for L in {1, 2, 3, 4, 5, 29 - start, 30 - start, 2 * ncol} if 1 <= L <= 2 * ncol)


def _specs(ncol):
    """name -> (the line's hashes in order, each a list of column kinds from column 0 on; the index of the hash the name stands for)"""
    s = {}
    for start in range(33):
        f = _filler(start, ncol)
        for L in _range_lengths(start, ncol):
            s[f"r{start}_{L}"] = (f + [_kinds(L, ncol)], len(f))
        if start < 28:        # the hash ends where a line of 29 would: three more words behind it make it a line of 28
            s[f"r{start}_{29 - start}_more"] = (f + [_kinds(min(29 - start, 2 * ncol), ncol), [S] * 3], len(f))
    for start in STARTS_SECOND:
        for name, kinds in PATTERNS.items():
            s[f"s{start}_{name}"] = (_filler(start, ncol) + [kinds], len(_filler(start, ncol)))
    for i in range(8):
        s[f"l8_{i}"] = (_filler(i, ncol) + [[S, LST, S]], 1 if i else 0)          # the list at word 4 + i: lanes 1, 1, 1, 1, 2, 2, 2, 2
        s[f"l8s_{i}"] = ([[S], [LST, S]], 1)                                       # the list at word 4: lane 1's first register of the line
    s["ll2"] = ([[S], [LST, LST, S]], 1)                                           # words 4, 5 lists: lane 1
    s["ll3"] = ([[S], [LST, LST, LST, S]], 1)                                      # words 4, 5, 6
    s["l_last"] = (_filler(20, ncol) + [_kinds(8, ncol - 1) + [LST]], len(_filler(20, ncol)))            # 29 words: the list is word 31
    s["l_last28"] = (_filler(20, ncol) + [_kinds(7, ncol - 1) + [LST], [S] * 3], len(_filler(20, ncol)))  # a line of 28: the list is word 30
    s["l_ext"] = (_filler(24, ncol) + [_kinds(7, ncol - 1) + [LST]], len(_filler(24, ncol)))             # four words inline, the list in ext
    return s


class World:
    def __init__(self, fpx, oracle, Pair, ctx, ncol, memory, per=300, seed=1409):
        self.ncol, self.hv = ncol, 64 // ncol
        rng = self.rng = np.random.default_rng(seed + ncol)
        firsts = [1 + c * per for c in range(ncol)]
        posts = [[] for _ in range(ncol)]
        u64 = np.uint64

        def add(h, spec, salt):
            """spec: (column, kind) pairs"""
            for col, kind in spec:
                docs = firsts[col] + 10 + (np.arange(kind) + salt) % POOL
                posts[col].append((u64(h) << u64(32)) | docs.astype(u64))

        self.line, self.hash, self.all = {}, {}, []
        for c, (name, (hashes, t)) in enumerate(_specs(ncol).items()):
            base = BASE + c * 64
            assert len(hashes) <= self.hv, name
            self.line[name] = [base + j for j in range(len(hashes))]
            self.hash[name] = base + t
            for j, kinds in enumerate(hashes):
                assert len(kinds) <= ncol, name
                add(base + j, list(enumerate(kinds)), 3 * j)      # (a hash's docs differ from its neighbours' in the line, and recur from line to line)
                self.all.append(base + j)
        for j, h in enumerate(TOP):
            add(h, list(enumerate([D, S, LST, S][: 2 + j % 3])), j)
        for j in range(self.hv):                 # the group's first line has every hash value, in the first columns
            add(LOW + j, [(0, D), (1, S)], j)
        self.hots = [HOTS + 977 * k for k in range(48 // ncol)]
        noise = []
        for c in range(ncol):
            docs = np.arange(firsts[c], firsts[c] + per, dtype=u64)
            h = rng.integers(1 << 20, (1 << 32) - (1 << 20), (per, 24), dtype=u64)
            noise.append(((h << u64(32)) | docs[:, None]).ravel())
            for k in self.hots:
                posts[c].append((u64(k) << u64(32)) | docs[:HOT_DOCS])
        # gap positions of column GAP_COL: the hash values between a block's last hash and the next block's first.  No made hash has the
        # column so far at such a value, and what the other columns get there leaves this column's blocks as they are.
        ids = [np.arange(firsts[c], firsts[c] + per, dtype=np.uint32) for c in range(ncol)]
        items = np.unique(np.concatenate([noise[GAP_COL]] + posts[GAP_COL]))
        blocks, index = oracle.build_blocks(items, firsts[GAP_COL], 512)
        alone = oracle.Snapshot([oracle.file_segment(blocks, 512, index, firsts[GAP_COL], firsts[GAP_COL] + per - 1, GAP_COL + 1, ids[GAP_COL])], [])
        self.gaps = []
        for b in range(1, len(index)):
            for h in (int(index[b]) - 1, int(index[b]) + 1):
                if len(self.gaps) < 4 and (1 << 20) < h < BASE:
                    _, ost = alone.search(np.array([h], dtype=np.uint32), 10, 1, 0, with_stats=True)
                    if ost.scanned_blocks == 0 and ost.scanned_docs == 0:
                        self.gaps.append(h)
        assert len(self.gaps) == 4, "no gap positions"
        for v, h in enumerate(self.gaps):        # v docs, the gap mark, two lists, a doc: the gap and the lists in one lane for three of the four
            add(h, [(c, S) for c in range(v)] + [(5, LST), (6, LST), (7, S)], v)
        self.pair = p = Pair(ctx)
        self.first_hash, self.last_hash = [], []
        for c in range(ncol):
            items = np.unique(np.concatenate([noise[c]] + posts[c]))
            p.add_file(items, firsts[c], firsts[c] + per - 1, c + 1, ids[c])
        if memory:
            docs = np.arange(ncol * per + 1, ncol * per + 41, dtype=u64)
            h = rng.integers(0, 1 << 32, (40, 24), dtype=u64)
            extra = [(u64(t) << u64(32)) | docs[:3] for t in self.all[::7]]
            items = np.unique(np.concatenate([((h << u64(32)) | docs[:, None]).ravel()] + extra))
            p.add_memory(items, int(docs[0]), int(docs[-1]), ncol + 1, docs.astype(np.uint32))
        p.finish()
        assert all(g.direct and g.grouped for g in p.gpu_segs[:ncol]), [g.layout_reason for g in p.gpu_segs[:ncol]]

    def noise(self, n):
        return self.rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def query(self, n, placed):
        """n hashes of noise, the made hashes `placed` {position: hash} among them"""
        q = self.noise(n)
        for at, h in placed.items():
            q[at] = h
        return q

    def spread(self, hashes, n=None, first=3, step=7):
        """the hashes `step` positions apart: other lanes of their groups, other groups, from 64 on another wave"""
        hashes = list(hashes)
        return self.query(n or max(64, first + step * len(hashes)), {first + step * i: h for i, h in enumerate(hashes)})

    def check(self, fpx, queries, two=False, fits=True, want=QUERY_WG):
        if fits:                             # (the records of a query have to fit its workgroup's array, or the batch goes the long way)
            for q in queries:
                _, ost = self.pair.osnap.search(q, with_stats=True)
                assert ost.scanned_docs < REC_CAP and len(q) <= 4096, (len(q), ost.scanned_docs)
        opts = [fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0)] + ([fpx.SearchOptions(max_results=40, min_score=6, min_score_pct=10)] if two else [])
        first = None
        for o in opts:
            got, st = self.pair.check(queries, o)
            assert st.path_flags & want == want, f"the batch did not take the path under test ({st.path_flags}, {want})"
            assert not st.path_flags & FILTERED, f"the filtered form ({st.path_flags})"
            first = got if first is None else first
        return first


@pytest.fixture(scope="module", params=[16, 8])
def ncol(request):
    """(module-scoped: pytest runs every test of one world before it turns to the next)"""
    return request.param


@pytest.fixture(scope="module")
def env():
    from fpx_testlib import fpx, oracle, Pair
    ctx = fpx.Context(0)
    made = {}                                # ONE world at a time: a packed group's lines take 69 - 137 GB of the device whatever its items
    prev = os.environ.get("FPX_DIRECT_MIN_ITEMS")

    def world(ncol, memory=False):
        if (ncol, memory) not in made:
            made.clear()
            gc.collect()
            os.environ["FPX_DIRECT_MIN_ITEMS"] = "0"
            ctx.set_option("group_packed", 1)
            try:
                made[(ncol, memory)] = World(fpx, oracle, Pair, ctx, ncol, memory)
            finally:
                ctx.set_option("group_packed", -2)
                if prev is None:
                    del os.environ["FPX_DIRECT_MIN_ITEMS"]
                else:
                    os.environ["FPX_DIRECT_MIN_ITEMS"] = prev
        return made[(ncol, memory)]

    yield fpx, world, ctx
    made.clear()
    gc.collect()
    for name in ("hot_wg", "query_wg"):
        ctx.set_option(name, -1)
    ctx.set_option("group_packed", -2)


def _range_queries(w, starts):
    """a query per start: its lengths' hashes seven positions apart"""
    return [w.spread([w.hash[n] for n in w.hash if n.startswith(f"r{start}_")]) for start in starts]


def _second_queries(w):
    return [w.spread([w.hash[f"s{start}_{name}"] for name in PATTERNS]) for start in STARTS_SECOND]


def _list_queries(w):
    l8, l8s = [w.hash[f"l8_{i}"] for i in range(8)], [w.hash[f"l8s_{i}"] for i in range(8)]
    qs = [w.query(64, {16 + i: h for i, h in enumerate(l8)}),               # a group whose eight lines each hold a list
          w.query(64, {40 + i: h for i, h in enumerate(l8s)}),              # ... all eight in ONE lane's registers
          w.query(300, {8: l8s[0], 13: l8s[1]}),                            # two and three lists in one lane, different lines of the group
          w.query(300, {264: l8s[2], 266: l8s[3], 271: l8s[4]}),
          w.query(64, {9: w.hash["ll2"]}), w.query(64, {63: w.hash["ll3"]}),       # ... of one line
          w.query(64, {9: w.hash["ll2"], 11: w.hash["ll3"], 14: l8s[5]}),          # six lists in one lane
          w.spread([w.hash[n] for n in ("l_last", "l_last28", "l_ext")])]
    qs += [w.query(64, {5 + 8 * v: h}) for v, h in enumerate(w.gaps)]       # a gap mark before two lists
    qs.append(w.query(64, {24 + v: h for v, h in enumerate(w.gaps)}))       # ... in four lines of one group
    qs.append(w.query(64, {24: w.gaps[1], 25: w.hash["ll3"], 26: w.gaps[2], 27: l8s[6]}))
    return qs


def _address_queries(w):
    rich = w.hash[f"r9_{2 * w.ncol}"]
    low = [LOW + j for j in range(w.hv)]
    qs = [w.query(300, {**{2 + 9 * i: h for i, h in enumerate(TOP)}, **{5 + 9 * i: h for i, h in enumerate(low)}, 290: rich}),
          w.query(len(TOP) + len(low), dict(enumerate(list(TOP) + low)))]
    # every hash that load instruction 3 reads for -- lane 3 of every group -- is a duplicate of the query's first hash but one
    for n, keep in ((64, 19), (256, 131), (300, 259)):
        q = w.query(n, {0: rich, keep: w.hash["s2_alt"]})
        for at in range(3, n, 8):
            if at != keep:
                q[at] = rich
        qs.append(q)
    qs.append(np.full(64, rich, dtype=np.uint32))
    qs.append(w.query(1, {0: rich}))
    for n in (255, 256, 257):
        qs.append(w.query(n, {0: w.hash["s1_all"], n // 2: TOP[2], n - 2: LOW + 1, n - 1: rich}))
    return qs


def test_range_word(env, ncol):
    fpx, world, _ = env
    w = world(ncol)
    got = w.check(fpx, _range_queries(w, range(33)))
    assert all(len(g) > 1 for g in got), "the made hashes' docs reach the floor"
    # one hash per query: a failure names the case
    names = [n for n in w.hash if n.startswith("r")]
    w.check(fpx, [w.query(9, {c % 9: w.hash[n]}) for c, n in enumerate(names)])


def test_second_word_word(env, ncol):
    fpx, world, _ = env
    w = world(ncol)
    w.check(fpx, _second_queries(w), two=True)
    names = [f"s{start}_{name}" for start in STARTS_SECOND for name in PATTERNS]
    w.check(fpx, [w.query(17, {c % 17: w.hash[n]}) for c, n in enumerate(names)])


def test_list_picking(env, ncol):
    fpx, world, _ = env
    w = world(ncol)
    got = w.check(fpx, _list_queries(w), two=True)
    assert any(len(g) > 1 for g in got)


def test_addresses_duplicates_and_lengths(env, ncol):
    fpx, world, _ = env
    w = world(ncol)
    got = w.check(fpx, _address_queries(w), two=True)
    assert all(len(g) > 1 for g in got[:2]), "the lines at both ends of the hash space were found"


def test_redone_in_classes(env, ncol):
    """a query of all of the above and the hot hashes: more records than the array holds, redone in doc classes (hot_wg = 1)"""
    fpx, world, ctx = env
    w = world(ncol)
    made = [w.hash[n] for n in w.hash if n.startswith(("r", "s"))][::5] + [w.hash[n] for n in ("ll2", "ll3", "l_last", "l_last28", "l_ext")] + w.gaps + list(TOP)
    heavy = np.concatenate([np.asarray(made + w.hots, dtype=np.uint32), w.noise(100)])
    w.rng.shuffle(heavy)
    _, ost = w.pair.osnap.search(heavy, with_stats=True)
    assert ost.scanned_docs > REC_CAP and len(heavy) <= 1024
    try:
        ctx.set_option("hot_wg", 1)
        w.check(fpx, [_range_queries(w, [7])[0], heavy, _list_queries(w)[0]], fits=False, want=QUERY_WG | REDONE)
    finally:
        ctx.set_option("hot_wg", -1)


def test_next_to_a_memory_segment(env):
    fpx, world, _ = env
    w = world(8, memory=True)
    qs = _range_queries(w, (0, 1, 5, 13, 24, 27, 28, 32)) + _second_queries(w)[1::2] + _list_queries(w) + _address_queries(w)
    got = w.check(fpx, qs)
    assert any(len(g) > 1 for g in got)
