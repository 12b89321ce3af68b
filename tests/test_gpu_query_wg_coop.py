"""The unfiltered rounds of k_search_query (csrc/fpx_qsearch.hpp): EIGHT LANES TO A LINE.  A hash's line is fetched once and whole by the
eight lanes of its lane's group (load instruction k: the line of the hash that lane k of the group holds, lane `sub` words 4 sub .. 4 sub + 3);
the hash's own lane does the head's arithmetic and the per-hash statistics, start / words count / inline limit / second-word mask go back
to the group, and every lane classifies its own four words of each of the group's eight lines.  Against the oracle through Pair.check:
results and every query's scanned blocks / docs; every batch asserts path_flags & 64 (a query per workgroup), and every query's records
are counted on the CPU to stay under the workgroup's record array (the oracle-equal path is the kernel under test).

The data is made for it: LINES of their own, 64 hash values apart, whose hashes hold a given number of columns / doubles / a list.

* a RICH hash -- words before it in its line, doubles, a list reference among its inline words, its tail in `ext` -- at each of the 256
  positions of a round: every lane of every wave, every lane of a group, every group of a load instruction;
* query lengths 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 1000, 1025: partial groups, partial waves, partial rounds, a third pair of rounds;
* two, three and four hashes of one query in the SAME line: in one group, in different groups of one load instruction, in different
  rounds; a duplicate of the rich hash inside one group;
* hashes of 13 .. 2 x columns words (tasks of the per-lane walk), at the line's start and behind three words;
* a hash that starts at or behind the line's inline limit (everything in `ext`); a line of 28 inline words with the offset of the rest in
  word 31 next to a line of 29 inline words whose word 31 is a doc;
* hashes below and above every column's hash range, each column's first and last hash and their neighbours, 0 and 0xFFFFFFFF;
* an absent hash in a populated line; duplicates and lanes past the query's end next to a group's first line that has every hash value;
* the same lines next to a memory segment (the MEM instantiations).

Deliberate mutations of the kernel that these tests were seen to catch (each one alone, every test of this file run against it): the line
fetched for the hash of the group's lane k ^ 1 instead of lane k (13 of 13 tests fail); word 31 of an overflowing line walked as a doc --
the inline limit taken as 29 -- (12 of 13); the absent-column blocks of a hash added eight times, as if by every lane of the group (13); the
position of a lane's first word off by one, 4 sub - 2 (13); a group whose hash is no probe walking the line it read -- records only, its
tasks held back -- (13: such a group reads the group's FIRST line, the line of hashes 0 .. HV - 1, which these worlds fill: LOW)."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = 0x30000000             # the made lines start here, 64 hash values apart
POOL = 4                      # docs per column that the made hashes draw from
LOW = 0                       # the group's first line: a group's lines start where its first chunk of 2^26 hash values does
REC_CAP = 8192                # csrc/fpx_qsearch.hpp: QS_REC_CAP
LENGTHS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 1000, 1025)


def _specs(ncol):
    """name -> the line's hashes in order: (columns k, doubles d, column position of a list or None) or None (absent), and the index of
    the hash the name stands for"""
    s = {}
    if ncol == 16:
        s["rich"] = ([(9, 0, None), (16, 6, 5), None, None], 1)                  # start 9, 22 words: 19 inline, 3 in ext
        s["rich_ext_list"] = ([(9, 0, None), (16, 6, 15), None, None], 1)        # ... its list reference in ext
        before28 = [(16, 12, None)]
        s["all_ext"] = ([(16, 16, None), (5, 2, None)], 1)                       # start 32 > 28
    else:
        s["rich"] = ([(8, 8, None), (3, 0, None), (8, 6, 2)] + [None] * 5, 2)    # start 19, 13 words: 9 inline, 4 in ext
        s["rich_ext_list"] = ([(8, 8, None), (3, 0, None), (8, 6, 7)] + [None] * 5, 2)
        before28 = [(8, 8, None), (8, 4, None)]
        s["all_ext"] = ([(8, 8, None), (8, 8, None), (5, 2, None)], 2)
    n28 = len(before28)
    s["start_at_limit"] = (before28 + [(4, 1, None)], n28)                       # 28 + 5 words: start == inl == 28
    s["line_of_30"] = (before28 + [(2, 0, None)], n28)                           # 28 inline, word 31 the offset of the other two
    s["line_of_29"] = (before28 + [(1, 0, None)], n28)                           # 29 inline: word 31 is a doc
    s["same"] = ([(3, 1, None), (4, 0, None), (2, 2, None), (3, 0, None)], 0)    # four hashes of a few words in one line
    for w in range(13, 2 * ncol + 1):
        for form, (k, d) in enumerate(((min(w, ncol), w - min(w, ncol)), ((w + 1) // 2, w // 2))):
            s[f"w{w}_{form}"] = ([(k, d, None)], 0)
            s[f"w{w}_{form}_after3"] = ([(3, 0, None), (k, d, None)], 1)
    return s


class World:
    def __init__(self, fpx, Pair, ctx, ncol, memory, per=400, seed=911):
        self.ncol = ncol
        rng = self.rng = np.random.default_rng(seed + ncol)
        firsts = [1 + s * per for s in range(ncol)]
        posts = [[] for _ in range(ncol)]

        def words(h, c, k, d, lp):
            cols = sorted((c + i) % ncol for i in range(k))
            dbl = set(cols[(c + i) % k] for i in range(d)) if lp is None else set(cols[:d]) - {cols[lp]}
            for i, col in enumerate(cols):
                pool = firsts[col] + 10 + (np.arange(POOL) + c) % POOL
                n = (3 + c % 2) if (lp is not None and i == lp) else (2 if col in dbl else 1)
                posts[col].append((np.uint64(h) << np.uint64(32)) | pool[:n].astype(np.uint64))

        self.line, self.hash, self.all = {}, {}, []
        for c, (name, (hashes, t)) in enumerate(_specs(ncol).items()):
            base = BASE + c * 64
            self.line[name] = [base + j for j in range(len(hashes))]
            self.hash[name] = base + t
            for j, spec in enumerate(hashes):
                if spec is not None:
                    words(base + j, c, *spec)
                    self.all.append(base + j)
        # the group's FIRST line -- the one a group of lanes whose hash is no probe reads -- has every hash value, in the first columns
        for j in range(64 // ncol):
            words(LOW + j, 0, 2, 1, None)
        self.pair = p = Pair(ctx)
        self.first_hash, self.last_hash = [], []
        for s in range(ncol):
            docs = np.arange(firsts[s], firsts[s] + per, dtype=np.uint64)
            h = rng.integers(1 << 20, (1 << 32) - (1 << 20), (per, 24), dtype=np.uint64)
            items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel()] + posts[s]))
            p.add_file(items, firsts[s], firsts[s] + per - 1, s + 1, np.arange(firsts[s], firsts[s] + per, dtype=np.uint32))
            self.first_hash.append(int(items[0] >> np.uint64(32)))
            self.last_hash.append(int(items[-1] >> np.uint64(32)))
        if memory:
            docs = np.arange(ncol * per + 1, ncol * per + 41, dtype=np.uint64)
            h = rng.integers(0, 1 << 32, (40, 24), dtype=np.uint64)
            extra = [(np.uint64(t) << np.uint64(32)) | docs[:3] for t in self.all[::7]]
            items = np.unique(np.concatenate([((h << np.uint64(32)) | docs[:, None]).ravel()] + extra))
            p.add_memory(items, int(docs[0]), int(docs[-1]), ncol + 1, docs.astype(np.uint32))
        p.finish()
        assert all(g.direct and g.grouped for g in p.gpu_segs[:ncol]), [g.layout_reason for g in p.gpu_segs[:ncol]]
        # some made hashes for the other lanes of a query
        self.company = [self.hash[n] for n in ("rich_ext_list", "all_ext", "start_at_limit", "line_of_30", "line_of_29", f"w{2 * ncol}_0", "w13_1_after3")] \
            + self.line["same"] + [self.line["rich"][0], self.line["rich"][-1]]          # (the last one: absent in a populated line)

    def noise(self, n):
        return self.rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def query(self, n, placed, company=True):
        """n hashes of noise, the made hashes `placed` {position: hash} among them, and (company) others at every 17th free position"""
        q = self.noise(n)
        if company:
            for i, h in enumerate(self.company):
                at = (7 + 17 * i) % n
                if at not in placed:
                    q[at] = h
        for at, h in placed.items():
            q[at] = h
        return q

    def check(self, fpx, queries, opts=None):
        for q in queries:                    # (the records of a query have to fit its workgroup's array, or the batch goes the long way)
            _, ost = self.pair.osnap.search(q, with_stats=True)
            assert ost.scanned_docs < REC_CAP and len(q) <= 4096, (len(q), ost.scanned_docs)
        first = None
        for o in opts or [fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0), fpx.SearchOptions(max_results=40, min_score=6, min_score_pct=10)]:
            got, st = self.pair.check(queries, o)
            assert st.path_flags & 64, f"the batch did not run k_search_query ({st.path_flags})"
            assert not st.path_flags & 256, f"the filtered form ({st.path_flags})"
            first = got if first is None else first
        return first                         # (the results under the first options: the lowest floor)


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
                made[(ncol, memory)] = World(fpx, Pair, ctx, ncol, memory)
            finally:
                ctx.set_option("group_packed", -2)
                if prev is None:
                    del os.environ["FPX_DIRECT_MIN_ITEMS"]
                else:
                    os.environ["FPX_DIRECT_MIN_ITEMS"] = prev
        return made[(ncol, memory)]

    yield fpx, world
    made.clear()
    gc.collect()
    ctx.set_option("query_wg", -1)
    ctx.set_option("group_packed", -2)


def test_rich_hash_in_every_lane_of_every_wave(env, ncol):
    fpx, world = env
    w = world(ncol)
    rich = w.hash["rich"]
    got = w.check(fpx, [w.query(256, {p: rich}) for p in range(256)], [fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0)])
    assert all(len(g) > 1 for g in got), "the made hashes' docs reach the floor"
    # ... and alone among noise: nothing else in its group, its wave, its round
    w.check(fpx, [w.query(256, {p: rich}, company=False) for p in (0, 7, 8, 63, 64, 200, 255)] + [w.query(1, {0: rich}, company=False)])


def test_query_lengths(env, ncol):
    fpx, world = env
    w = world(ncol)
    rich = w.hash["rich"]
    qs = []
    for n in LENGTHS:
        qs.append(w.query(n, {n - 1: rich}))                                     # the last lane of a partial group / wave / round
        qs.append(w.query(n, {0: rich, n // 2: w.hash["all_ext"], n - 1: w.hash["line_of_29"]}))
    got = w.check(fpx, qs)
    assert any(len(g) > 1 for g in got)


def test_hashes_of_one_line_and_duplicates(env, ncol):
    fpx, world = env
    w = world(ncol)
    same, rich = w.line["same"], w.hash["rich"]
    qs = []
    for m in (2, 3, 4):
        qs.append(w.query(300, {16 + i: same[i] for i in range(m)}, company=False))               # one group
        qs.append(w.query(300, {3 + 8 * i: same[i] for i in range(m)}, company=False))            # different groups of one load instruction
        qs.append(w.query(300, {5 + 64 * i: same[i] for i in range(m)}, company=False))           # ... of different waves
        qs.append(w.query(1000, {5 + 256 * i: same[i] for i in range(m)}, company=False))         # different rounds
        qs.append(w.query(300, {40 + 9 * i: same[i] for i in range(m)}))                          # different groups, different instructions
    # the rich hash, the first hash of its line and the absent one in one group; a duplicate of the rich hash inside one group, in
    # another group, in another round
    qs.append(w.query(300, {32: w.line["rich"][0], 34: rich, 39: w.line["rich"][-1]}))
    qs.append(w.query(200, {18: rich, 21: rich}))
    qs.append(w.query(200, {18: rich, 21: rich, 29: rich, 190: rich}, company=False))
    qs.append(w.query(600, {18: rich, 18 + 256: rich, 19 + 512: rich}))
    qs.append(np.full(64, rich, dtype=np.uint32))
    got = w.check(fpx, qs)
    assert any(len(g) > 1 for g in got)


def test_hashes_of_13_and_more_words(env, ncol):
    fpx, world = env
    w = world(ncol)
    names = [n for n in w.hash if n.startswith("w")]
    assert {int(n[1:].split("_")[0]) for n in names} == set(range(13, 2 * ncol + 1))
    targets = np.asarray([w.hash[n] for n in names], dtype=np.uint32)
    order = w.rng.permutation(len(targets))
    qs = [w.query(260, {int(3 + 11 * i): int(t) for i, t in enumerate(targets[order[s:s + 8]])}, company=False) for s in range(0, len(order), 8)]
    w.check(fpx, qs)
    # one case per query: a failure names the case
    w.check(fpx, [w.query(70, {c % 64: int(t)}, company=False) for c, t in enumerate(targets)], [fpx.SearchOptions(max_results=500, min_score=3, min_score_pct=0)])


def test_line_ends_and_words_in_ext(env, ncol):
    fpx, world = env
    w = world(ncol)
    names = ("all_ext", "start_at_limit", "line_of_30", "line_of_29", "rich", "rich_ext_list")
    qs = [w.query(100, {9: w.hash[n]}, company=False) for n in names]
    qs += [w.query(100, {9 + i: h for i, h in enumerate(w.line[n])}, company=False) for n in names]          # ... with the hashes before them
    qs.append(w.query(400, {13 * i: w.hash[n] for i, n in enumerate(names)}))
    # the two lines next to one another in a group: 28 inline words + the offset, 29 inline words
    qs.append(w.query(64, {24: w.hash["line_of_30"], 25: w.hash["line_of_29"], 26: w.line["line_of_30"][0], 27: w.line["line_of_29"][0]}, company=False))
    w.check(fpx, qs)


def test_hash_ranges_and_absent_hashes(env, ncol):
    fpx, world = env
    w = world(ncol)
    edge = [0, 1, 1000, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFF000]
    for f, l in zip(w.first_hash, w.last_hash):
        edge += [f - 1, f, f + 1, l - 1, l, l + 1]
    # (the first line's hashes are in the first two columns only: hashes below 2^20 lie inside their ranges and below all the others')
    assert min(w.first_hash) == LOW and 1000 < max(w.first_hash) and max(edge) > max(w.last_hash)
    edge = np.asarray([e for e in edge if 0 <= e <= 0xFFFFFFFF], dtype=np.uint32)
    absent = [w.line["rich"][-1], w.line["same"][0] + 4 if ncol == 8 else w.line["all_ext"][0] + 3, w.line["line_of_29"][0] + 64 // ncol - 1]
    qs = [np.concatenate([edge, w.noise(100)]), w.query(300, {2 * i: int(h) for i, h in enumerate(edge)}),
          w.query(100, {10 + i: h for i, h in enumerate(absent)}, company=False), w.query(100, {10 + 8 * i: h for i, h in enumerate(absent)})]
    w.check(fpx, qs)


def test_next_to_a_memory_segment(env):
    fpx, world = env
    w = world(8, memory=True)
    rich = w.hash["rich"]
    qs = [w.query(256, {p: rich}) for p in range(0, 256, 37)] + [w.query(n, {n - 1: rich, 0: w.hash["all_ext"]}) for n in (9, 65, 257, 1025)]
    qs.append(np.asarray(w.all, dtype=np.uint32)[::3])
    got = w.check(fpx, qs)
    assert any(len(g) > 1 for g in got)
