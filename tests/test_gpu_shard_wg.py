"""Option shard_wg (csrc/fpx_qsearch.hpp: k_search_window; csrc/fpx_search.hip: shard_probe_impl): a step of the sharded bin protocol on
a rank whose snapshot is ONE packed group with its hash window (+ memory segments behind their table) walks the window a QUERY PER
WORKGROUP -- dedup over the whole query, the window's hashes walked, the query's hit records copied into its bin of 8 queries with one
reservation -- instead of making, ordering and probing the window's keys.  The bins are the protocol's as they were, so every case
compares the step under the option against the step under 0 (every bin's records, nulls dropped and sorted; the travelling counts'
width bit; blocks, docs, probes and hits summed over the ranks against the unsharded batch's), and the results after fpx_shard_score
over what the all-to-all would deliver against the unsharded snapshot's and the oracle's, query by query.  fpx_stats.path_flags bit 14
(with bit 6) says which way a rank went.

The worlds are tests/test_gpu_hashshard.py's (_sharded_world: 'rank' r of N holds window r of every segment, cut on the device), built
under group_packed = 1, FPX_DIRECT_MIN_ITEMS = 0 and FPX_FUSE_MIN = 1; a rank's slices are asserted to be ONE packed group.  A packed
group's lines cost device memory by the hash space however few its docs: a world is built once per module and case, and released.

On a library without the feature the option's name is refused: every case fails at its first set_option."""
import contextlib
import functools
import os

import numpy as np
import pytest

import wg_harness as wg
from wg_harness import HOT1, HOT8

pytestmark = pytest.mark.gpu

WALKED, QUERY_WG = 1 << 14, 64
DEDUP_MAX = 2048
PATTERN = 0x7EEEEEEE7EEEEEEE                         # a cell that is neither records (doc 0x0FDDDDDD, query 0x7EEEEEEE: not of these worlds) nor all ones
SEED, H, PER, S = 31, 64, 5000, 3
# case 6's postings at the edges of rank 1 of 4's window [0x40000000, 0x7FFFFFFF] (and the hash the dedup set keeps apart): docs 11, 12, 13 of segment 0
EDGES = (0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0x80000000)
ONES = 0xFFFFFFFF


# ---- worlds ---------------------------------------------------------------------------------------------------------------------

def _world_data(fpx, rng, first=1, again=True, edges=False):
    """test_gpu_hashshard.py's segments: S x PER docs x H hashes, hot pool; again: later segments re-insert 200 older docs, 20 of them
    as tombstones.  edges: segment 0 also holds EDGES and ONES, each the hash of docs first + 10 .. first + 12"""
    data = []
    for s in range(S):
        lo = first + s * PER
        ids = np.arange(lo, lo + PER, dtype=np.uint64)
        older = np.arange(first, lo, dtype=np.uint64)
        if edges:                                                     # (the edge postings' docs stay live)
            older = np.setdiff1d(older, np.arange(first + 10, first + 13, dtype=np.uint64))
        extra = np.sort(rng.choice(older, 200, replace=False)) if s and again else np.zeros(0, np.uint64)
        all_ids = np.concatenate([extra, ids])
        h = fpx.synth.synth_hashes(SEED + s, all_ids, H, 1).astype(np.uint64)
        items = ((h << np.uint64(32)) | all_ids[:, None]).ravel()
        if edges and s == 0:
            items = np.concatenate([items] + [wg.post(e, [first + 10, first + 11, first + 12]) for e in EDGES + (ONES,)])
        items = np.unique(items)
        alive = np.ones(len(all_ids), np.uint8)
        if s and again:
            alive[:20] = 0
            items = items[~np.isin(items & np.uint64(0xFFFFFFFF), all_ids[:20])]
        data.append((items, int(all_ids.min()), int(all_ids.max()), all_ids.astype(np.uint32), alive))
    return data


class Ranks:
    """the unsharded index (GPU + oracle) and one reader per 'rank': the rank's window of every segment, cut on the device, and a copy of
    every memory segment -- the same items on every rank, as the ABI prescribes"""

    def __init__(self, env, world, data, changes=()):
        fpx, oracle, Pair, ctx = env
        self.fpx, self.ctx, self.world = fpx, ctx, world
        self.full = Pair(ctx)
        for s, (items, lo, hi, ids, alive) in enumerate(data):
            self.full.add_file(items, lo, hi, s + 1, ids, alive)
        mems = []
        for c in changes:
            commit = len(self.full.gpu_segs) + 1
            self.full.add_memory_changes(c, commit)
            m = self.full.orc_mem[-1]
            mems.append((m, commit) + tuple(m.docs()))
        self.full.finish()
        assert all(g.grouped for g in self.full.gpu_segs[:len(data)])
        self.max_doc = max([hi for _, _, hi, _, _ in data] + [m.max_doc_id for m, _, _, _ in mems])
        self.readers, self.segs = [], []
        for r in range(world):
            lo_excl = None if r == 0 else (r << 32) // world - 1
            hi_incl = None if r == world - 1 else ((r + 1) << 32) // world - 1
            segs = []
            for s, (items, lo, hi, ids, alive) in enumerate(data):
                blocks, index = oracle.build_blocks(items, lo, 512)
                whole = fpx.FileSegment(ctx, blocks, 512, index, lo, hi, s + 1, ids, alive)
                segs.append(whole.window(lo_excl, hi_incl))
                whole.release()
            files = len(segs)
            for m, commit, ids, alive in mems:
                segs.append(fpx.MemorySegment(ctx, m.items(), m.min_doc_id, m.max_doc_id, commit, ids, alive))
            self.readers.append(fpx.IndexReader(fpx.Segments(ctx, segs)))
            self.segs.append(segs)
            # the rank's slices formed ONE packed group with their window
            assert all(g.grouped for g in segs[:files]), [g.layout_reason for g in segs[:files]]
            info = segs[0].group_info()
            assert info["packed"] == 1 and info["columns"] == files, info

    def window(self, r):
        return (r << 32) // self.world, ((r + 1) << 32) // self.world - 1

    def release(self):
        for rd in self.readers + [self.full.reader]:
            rd.snapshot.release()
        for g in [g for segs in self.segs for g in segs] + self.full.gpu_segs:
            g.release()
        self.ctx.trim()


@pytest.fixture(scope="module")
def env():
    return wg.open_context()


@pytest.fixture(autouse=True)
def tidy(env, monkeypatch):
    """every file segment a direct-addressed candidate, a column of a group even alone, groups packed; the option itself and the paths'
    other switches at their fallbacks before and after"""
    ctx = env[3]
    names = ("shard_wg", "direct_min_items", "fuse_min")
    monkeypatch.setenv("FPX_DIRECT_MIN_ITEMS", "0")
    monkeypatch.setenv("FPX_FUSE_MIN", "1")
    wg.reset(ctx, names)
    ctx.set_option("direct_min_items", 0); ctx.set_option("fuse_min", 1); ctx.set_option("group_packed", 1)
    try:
        yield
    finally:
        wg.reset(ctx, names)


class _Kept:
    """the filtered world of cases 1, 2, 4 and 6, kept from one test to the next while they ask for the same number of ranks -- one world
    at a time: its lines are most of the device's memory"""
    w = None

    @classmethod
    def get(cls, env, world):
        if cls.w is None or cls.w.world != world:
            cls.drop()
            # _sharded_world's shape (re-inserted docs, tombstones: a filtered group); segment 0 carries case 6's edge postings
            cls.w = Ranks(env, world, _world_data(env[0], np.random.default_rng(world), edges=True))
        return cls.w

    @classmethod
    def drop(cls):
        if cls.w is not None:
            cls.w.release()
            cls.w = None


@pytest.fixture(scope="module", autouse=True)
def kept_world_goes_with_the_module():
    yield
    _Kept.drop()


@contextlib.contextmanager
def _made(env, world, data, changes=()):
    _Kept.drop()
    w = None
    try:
        w = Ranks(env, world, data, changes)
        yield w
    finally:
        if w is not None:
            w.release()


def _queries(fpx, first=1, B=150):
    flat, off, _ = fpx.synth.make_queries(SEED, 3, B, PER * S, H, query_len=300, dist=1, first_doc=first)
    flat = flat.copy()
    flat[5] = flat[4]                                                 # a duplicate hash inside a query
    return [flat[int(off[i]):int(off[i + 1])] for i in range(B)]


def _three(fpx):
    return (fpx.http_options(), fpx.SearchOptions(500, 3, 10), fpx.SearchOptions(3, 4, 100))


# ---- a step of the protocol -----------------------------------------------------------------------------------------------------

class Step:
    """fpx_shard_probe on every rank under shard_wg = `level`, the bins sized by the ranks' largest need.  sends[r] = (cells, counts) of
    rank r, stats[r] its fpx_stats, attempts: calls per rank (1: the first size was enough)"""

    def __init__(self, w, qb, level, cell_cap=16, fill=0):
        import torch
        fpx, world = w.fpx, w.world
        self.w, self.qb, self.bpr = w, qb, fpx.shard_bins_per_rank(qb.B, world)
        w.ctx.set_option("shard_wg", level)
        try:
            for self.attempts in range(1, 6):
                self.sends, self.stats, need_max = [], [], 0
                for r in range(world):
                    send = torch.full((world, self.bpr, cell_cap), fill, dtype=torch.int64, device="cuda")
                    counts = torch.zeros((world, self.bpr), dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()            # (torch fills on ITS stream; libfpx writes these on a stream of its own)
                    st, need = fpx.shard_probe(w.readers[r], qb, world, send.data_ptr(), cell_cap, counts.data_ptr())
                    assert tuple(send.shape) == (world, self.bpr, cell_cap)
                    if st is None:
                        assert need > cell_cap
                        need_max = max(need_max, need)
                        continue
                    self.sends.append((send, counts))
                    self.stats.append(st)
                if need_max == 0:
                    break
                cell_cap = need_max                                   # (all ranks use one bin size)
            assert need_max == 0
        finally:
            w.ctx.set_option("shard_wg", -1)
        self.cell_cap = cell_cap

    def totals(self):
        return tuple(sum(getattr(st, k) for st in self.stats) for k in ("scanned_blocks", "scanned_docs", "probes", "hits"))

    def flags(self):
        return [st.path_flags for st in self.stats]

    def cells(self, fill=None):
        """[rank][bin] -> (the bin's records, nulls dropped, sorted; narrow?).  Every record is checked to sit in its query's bin; fill: the
        cells behind a bin's count must still hold it, and none below may"""
        w, B, out = self.w, self.qb.B, []
        for send, counts in self.sends:
            c = counts.cpu().numpy().reshape(-1).astype(np.int64) & 0xFFFFFFFF
            narrow, c = (c >> 31) != 0, c & 0x7FFFFFFF                # bit 31 of a travelling count: the bin holds 4-byte records
            sv = send.cpu().numpy().reshape(w.world * self.bpr, self.cell_cap)
            row = []
            for b in range(w.world * self.bpr):
                if narrow[b]:                                         # doc << 3 | query-in-bin, two to a cell
                    assert c[b] <= 2 * self.cell_cap
                    every = sv[b].view(np.uint32)
                    recs = every[:c[b]]
                    if fill is not None:
                        assert (every[c[b]:] == fill & 0xFFFFFFFF).all() and not (recs == fill & 0xFFFFFFFF).any(), b
                    recs = np.sort(recs[recs != 0xFFFFFFFF])
                    assert (b * 8 + (recs & 7) < max(B, 8)).all() and (recs >> 3 <= w.max_doc).all()
                else:                                                 # query << 32 | doc
                    assert c[b] <= self.cell_cap
                    recs = sv[b, :c[b]]
                    if fill is not None:
                        assert (sv[b, c[b]:] == fill).all() and not (recs == fill).any(), b
                    recs = np.sort(recs[recs != -1])
                    assert ((recs >> 32) >> 3 == b).all()
                row.append((recs, bool(narrow[b])))
            out.append(row)
        return out

    def results(self):
        """fpx_shard_score on every rank over what the all-to-all would deliver -> the batch's {id, score} lists"""
        import torch
        w, qb, fpx = self.w, self.qb, self.w.fpx
        out, out_n, covered = np.zeros((qb.B, qb.cap, 2), np.uint32), np.zeros(qb.B, np.uint32), 0
        for d in range(w.world):
            recv = torch.stack([self.sends[r][0][d] for r in range(w.world)]).contiguous()
            rc = torch.stack([self.sends[r][1][d] for r in range(w.world)]).contiguous()
            torch.cuda.synchronize()
            out, out_n, q_lo, q_hi = fpx.shard_score(w.ctx, qb, w.world, d, recv.data_ptr(), self.cell_cap, rc.data_ptr(), out, out_n)
            assert q_lo == min(qb.B, d * self.bpr * 8)
            covered += q_hi - q_lo
        assert covered == qb.B                                        # every query is finished by exactly one rank
        return fpx.results_to_lists(out, out_n)


def _equal_cells(a, b):
    ca, cb = a.cells(), b.cells()
    assert len(ca) == len(cb)
    for r, (ra, rb) in enumerate(zip(ca, cb)):
        assert len(ra) == len(rb)
        for bn, ((xa, na), (xb, nb)) in enumerate(zip(ra, rb)):
            assert na == nb, (r, bn, na, nb)
            assert len(xa) == len(xb) and (xa == xb).all(), (r, bn, len(xa), len(xb))


def _compare(w, queries, opts, level, walked=True, cell_cap=16):
    """the step under `level` and under 0: equal cells, the ranks' sums == the unsharded batch's, results == the unsharded snapshot's ==
    the oracle's.  walked: every rank's bit 14 (with bit 6) under `level` -- or one flag per rank; under 0 both are clear"""
    fpx = w.fpx
    qb = fpx.QueryBatch(w.ctx, queries, opts)
    on, off = Step(w, qb, level, cell_cap), Step(w, qb, 0, cell_cap)
    print(f"shard_wg {level}: path_flags {on.flags()}, totals {on.totals()}, cell_cap {on.cell_cap}; 0: {off.flags()}, {off.totals()}, {off.cell_cap}")
    want = [walked] * w.world if isinstance(walked, bool) else list(walked)
    assert [((f & WALKED) != 0, (f & QUERY_WG) != 0) for f in on.flags()] == [(x, x) for x in want], (on.flags(), want)
    assert not any(f & (WALKED | QUERY_WG) for f in off.flags()), off.flags()
    assert all(f & 16 for f in on.flags() + off.flags())
    _equal_cells(on, off)
    o2, n2, st_full = fpx.search_resident(w.full.reader, qb)
    whole = (st_full.scanned_blocks, st_full.scanned_docs, st_full.probes, st_full.hits)
    assert on.totals() == whole and off.totals() == whole, (on.totals(), off.totals(), whole)
    got, got0, unsharded = on.results(), off.results(), fpx.results_to_lists(o2, n2)
    assert got == unsharded and got0 == unsharded
    for q, (hashes, o) in enumerate(zip(queries, qb.options)):
        expect = w.full.osnap.search(hashes, o.max_results, o.min_score, o.min_score_pct)
        assert got[q] == expect, (q, got[q][:4], expect[:4])
    on.got = got
    qb.release()
    return on, off


# ---- 1. parity at 2, 4 and 8 ranks, a filtered world; 2. value 1 keeps the pipeline there; 4. FPX_E_AGAIN; 6. window edges --------------
# (in the order of the worlds they share: 2 ranks, 4, 8)

def _parity(env, world):
    w, fpx = _Kept.get(env, world), env[0]
    for opts in _three(fpx):
        _compare(w, _queries(fpx), opts, 2)


def test_parity_on_a_filtered_world_at_2_ranks(env):
    _parity(env, 2)


def test_value_1_leaves_a_filtered_group_to_the_pipeline(env):
    w = _Kept.get(env, 2)
    _compare(w, _queries(w.fpx), w.fpx.SearchOptions(500, 3, 10), 1, walked=False)


def test_a_bin_over_its_capacity_says_what_it_needs(env):
    """cell_cap = 16 first: the call returns the need, the retry with the ranks' largest succeeds.  The send buffer holds a pattern before
    each call: after the succeeding one every cell behind a bin's count (records and pads) still holds it, and none below does"""
    w = _Kept.get(env, 2)
    fpx = w.fpx
    qb = fpx.QueryBatch(w.ctx, _queries(fpx), fpx.SearchOptions(500, 3, 10))
    on, off = Step(w, qb, 2, cell_cap=16, fill=PATTERN), Step(w, qb, 0, cell_cap=16, fill=PATTERN)
    for step in (on, off):
        assert step.attempts == 2 and step.cell_cap > 16, (step.attempts, step.cell_cap)
    assert on.cell_cap == off.cell_cap                                # (the same counts: the same need)
    assert all(f & WALKED for f in on.flags()) and not any(f & WALKED for f in off.flags())
    for ra, rb in zip(on.cells(fill=PATTERN), off.cells()):
        for (xa, na), (xb, nb) in zip(ra, rb):
            assert na == nb and len(xa) == len(xb) and (xa == xb).all()
    assert on.results() == off.results()
    qb.release()


def test_parity_on_a_filtered_world_at_4_ranks(env):
    _parity(env, 4)


def test_window_edges_and_odd_queries(env):
    """one batch: a query with rank 1's win_lo - 1, win_lo, win_hi and win_hi + 1, each the hash of a posting that exists; an empty query;
    a query whose hashes all lie outside rank 1's window (rank 1 stores nothing for it); 0xFFFFFFFF twice; one hash 40 times; a query of
    exactly DEDUP_MAX hashes; then ordinary ones -- and the batch's first 1, 7 and 9 queries alone (fewer bins than ranks)"""
    w = _Kept.get(env, 4)
    fpx = w.fpx
    rng = np.random.default_rng(66)
    lo, hi = w.window(1)
    assert (lo - 1, lo, hi, hi + 1) == EDGES
    plain = _queries(fpx)
    outside = plain[20][(plain[20] < lo) | (plain[20] > hi)]
    long_q = np.concatenate([plain[30][:H], wg.noise(rng, DEDUP_MAX - H)])
    queries = [np.array(EDGES + (7, 8), dtype=np.uint32), np.zeros(0, np.uint32), outside, np.array([ONES, ONES], dtype=np.uint32),
               np.full(40, int(plain[3][0]), dtype=np.uint32), long_q] + plain[:144]
    assert len(long_q) == DEDUP_MAX and len(outside) > 100 and len(queries) == 150
    opts = fpx.SearchOptions(500, 3, 10)                              # (an empty query's default floor is 0: the record protocol's)
    for B in (150, 1, 7, 9):
        on, _ = _compare(w, queries[:B], opts, 2)
        got = on.got
        assert got[0] == [(11, 4), (12, 4), (13, 4)], got[0]           # every edge posting counted once, on the rank that owns its hash
        if B >= 7:
            assert got[1] == [] and got[3] == []                      # (0xFFFFFFFF once after dedup: a score of 1, below the floor)
            cells = on.cells()
            # rank 1 reserved nothing for the query outside its window: no record of query 2 in its bin 0
            recs, narrow = cells[1][0]
            assert not ((recs & 7 if narrow else recs >> 32) == 2).any()
            # ... and the rank that owns 0xFFFFFFFF has query 3's three docs, once each
            recs, narrow = cells[3][0]
            assert ((recs & 7 if narrow else recs >> 32) == 3).sum() == 3


def test_parity_on_a_filtered_world_at_8_ranks(env):
    _parity(env, 8)


# ---- 2. an unfiltered world under 1 ---------------------------------------------------------------------------------------------

def test_value_1_walks_an_unfiltered_group(env):
    fpx = env[0]
    with _made(env, 2, _world_data(fpx, np.random.default_rng(2), again=False)) as w:
        for opts in _three(fpx)[:2]:
            _compare(w, _queries(fpx), opts, 1)


# ---- 3. the record width ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_doc", [0x1FFFFFFE, 0x1FFFFFFF, 0xFFFFFFFF])
def test_cells_at_the_record_width_threshold(env, max_doc):
    """4-byte records while the declared max doc is below 0xFFFFFFFF >> 3: a world whose last doc is 0x1FFFFFFE travels narrow, one whose
    last doc is 0x1FFFFFFF -- or 0xFFFFFFFF -- wide, whichever way the window is searched"""
    fpx = env[0]
    first = max_doc - S * PER + 1
    narrow_expected = os.environ.get("FPX_REC32", "1") != "0" and max_doc < 0x1FFFFFFF
    with _made(env, 2, _world_data(fpx, np.random.default_rng(2), first=first)) as w:
        assert w.max_doc == max_doc
        on, off = _compare(w, _queries(fpx, first), fpx.SearchOptions(500, 3, 10), 2)
        for step in (on, off):
            assert all(narrow == narrow_expected for row in step.cells() for _, narrow in row)


# ---- 5. memory segments ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 8])
def test_memory_segments_behind_their_table(env, world):
    """the world without re-inserts; every rank also holds two memory segments that write 50 docs again -- with hashes of the batch's
    queries -- and delete 10.  shard_wg = 2 walks (MEM); under 1 the cells are the same whichever path the group's state chooses"""
    fpx = env[0]
    queries = _queries(fpx)
    rng = np.random.default_rng(50 + world)
    docs = rng.choice(np.arange(1, S * PER, dtype=np.int64), 60, replace=False)
    changes = []
    for m in range(2):
        again, gone = docs[m * 25:(m + 1) * 25], docs[50 + m * 5:55 + m * 5]
        changes.append([("insert", int(d), [int(h) for h in queries[(7 * i + m) % 150][:40 + i]]) for i, d in enumerate(again)] +
                       [("delete", int(d)) for d in gone])
    with _made(env, world, _world_data(fpx, np.random.default_rng(world), again=False), changes) as w:
        for opts in _three(fpx)[:2]:
            _compare(w, queries, opts, 2)
        qb = fpx.QueryBatch(w.ctx, queries, fpx.SearchOptions(500, 3, 10))
        one, off = Step(w, qb, 1), Step(w, qb, 0)
        print("shard_wg 1 with memory segments: path_flags", one.flags())
        assert len({bool(f & WALKED) for f in one.flags()}) == 1       # (every rank's group is in the same state)
        _equal_cells(one, off)
        assert one.totals() == off.totals() and one.results() == off.results()
        qb.release()


def test_memory_segments_of_new_docs_leave_the_group_unfiltered(env):
    """two memory segments that only ADD docs supersede nothing: the group stays unfiltered and shard_wg = 1 walks it with the table (MEM
    without FILT)"""
    fpx = env[0]
    queries = _queries(fpx)
    changes = [[("insert", S * PER + 100 + 10 * m + i, [int(h) for h in queries[(11 * i + m) % 150][:50 + i]]) for i in range(10)] for m in range(2)]
    with _made(env, 2, _world_data(fpx, np.random.default_rng(2), again=False), changes) as w:
        on, _ = _compare(w, queries, fpx.SearchOptions(500, 3, 10), 1)
        assert any((S * PER + 100, 50) in r for r in on.got), "the memory segments' docs are not among the results"


# ---- 7. a query whose records outgrow the workgroup's array: the same call is answered by the pipeline, and the next 32 ---------------

def test_hand_back_and_back_off(env):
    """wg_harness's HOT8 and HOT1 postings (8000 + 1000 records, both in rank 0 of 2's window) and hashes of one doc each: a query of
    exactly 8192 records in rank 0's window is walked; one of 8193 hands rank 0's step to the pipeline inside the call -- bit 14 clear,
    the cells and results what they must be -- and rank 0's snapshot stays there for its next 32 calls.  Rank 1 walks throughout"""
    fpx, oracle, Pair, ctx = env
    rng = np.random.default_rng(1540)
    single0 = 0x70000000
    singles = np.array([single0 + 7919 * k for k in range(3500)], dtype=np.uint32)
    data = []
    for s in range(8):
        ids = np.arange(1 + s * 1200, 1 + (s + 1) * 1200, dtype=np.int64)
        extra = [(HOT8, ids[:1000])]
        if s == 0:
            extra.append((HOT1, ids[200:1200]))
        if s == 1:
            extra += [(int(h), ids[i % len(ids): i % len(ids) + 1]) for i, h in enumerate(singles)]
        data.append((wg.rand_items(rng, ids, 24, extra), int(ids.min()), int(ids.max()), ids.astype(np.uint32), None))
    with _made(env, 2, data) as w:
        assert max(HOT8, HOT1, int(singles.max())) <= w.window(0)[1]

        def records(p, q):                                            # the records rank 0's window gives the query
            return p.osnap.search(q[q <= w.window(0)[1]], 40, 1, 0, with_stats=True)[1].scanned_docs
        exact = functools.partial(wg.exact, records)
        items = [d[0] for d in data]
        plain = [wg.aimed(rng, items[i % 8], 300) for i in range(30)]
        plain = [q[(q != HOT8) & (q != HOT1)] for q in plain]
        fits, over = exact(w.full, rng, [HOT8], singles, 8192), exact(w.full, rng, [HOT8], singles, 8193)
        assert (records(w.full, fits), records(w.full, over)) == (8192, 8193)
        opts = fpx.SearchOptions(500, 3, 10)
        light = plain[:11] + [fits] + plain[11:]
        heavy = light[:20] + [over] + light[20:]
        on, _ = _compare(w, light, opts, 1, cell_cap=8192)            # 8192 records: walked on both ranks
        assert on.attempts == 1
        # call 1: 8193 records -- the call succeeds, the pipeline answered on rank 0; calls 2 .. 33 on rank 0's snapshot stay there
        on, _ = _compare(w, heavy, opts, 1, walked=[False, True], cell_cap=8192)
        assert on.attempts == 1
        import torch
        qb = fpx.QueryBatch(ctx, light, opts)
        bpr = fpx.shard_bins_per_rank(qb.B, 2)
        send = torch.zeros((2, bpr, 8192), dtype=torch.int64, device="cuda")
        counts = torch.zeros((2, bpr), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.set_option("shard_wg", 1)
        # (_compare's second step ran under 0: it neither tried nor counted.  Its first step made call 1; the 32 calls that do not try:)
        seen = []
        for call in range(2, 35):
            st, need = fpx.shard_probe(w.readers[0], qb, 2, send.data_ptr(), 8192, counts.data_ptr())
            assert st is not None, need
            seen.append(bool(st.path_flags & WALKED))
        assert seen == [False] * 32 + [True], seen                    # calls 2 .. 33 clear, call 34 walks again
        st, _ = fpx.shard_probe(w.readers[1], qb, 2, send.data_ptr(), 8192, counts.data_ptr())
        assert st.path_flags & WALKED
        qb.release()


# ---- 8. the one call -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 4])
def test_one_call_over_window_sharded_contexts(env, world):
    """fpx_sharded_snapshot_create_windows over `world` contexts on device 0 (tests/test_gpu_sharded_abi.py's way) on case 1's world:
    fpx_sharded_search_batch under shard_wg = 2 on every context gives every context the whole batch and walks its window -- results ==
    the unsharded snapshot's == the oracle's, bit 14, the unsharded scanned blocks and docs; under 0 the routed keys, the same results"""
    fpx, oracle, Pair, ctx0 = env
    import torch
    _Kept.drop()
    ndev = torch.cuda.device_count()
    ctxs = [fpx.Context(k % ndev) for k in range(world)]
    for c in ctxs:
        c.set_option("direct", 1); c.set_option("direct_min_items", 0); c.set_option("fuse_min", 1); c.set_option("group_packed", 1)
    full = Pair(ctxs[0])
    slices = [[] for _ in range(world)]
    for s, (items, lo, hi, ids, alive) in enumerate(_world_data(fpx, np.random.default_rng(world))):
        blocks, index = full.add_file(items, lo, hi, s + 1, ids, alive)
        for k, sl in enumerate(fpx.file_segment_windows(ctxs, blocks, 512, index, lo, hi, s + 1, ids, alive)):
            slices[k].append(sl)
    full.finish()
    sh = fpx.ShardedIndexReader(fpx.WindowShardedSegments(ctxs, slices))
    try:
        assert sh.snapshot.num_devices == world
        for row in slices:
            info = row[0].group_info()
            assert all(g.grouped for g in row) and info["packed"] == 1 and info["columns"] == S, info
        queries = _queries(fpx)
        for opts in _three(fpx):
            want, wst = full.check(queries, opts, with_stats=False)
            for level in (2, 0, 2):
                for c in ctxs:
                    c.set_option("shard_wg", level)
                got, st = sh.search_batch(queries, opts)
                print(f"shard_wg {level}: path_flags {st.path_flags}")
                assert got == want
                assert bool(st.path_flags & WALKED) == (level == 2) and st.path_flags & 16
                assert (st.scanned_blocks, st.scanned_docs, st.probes, st.hits) == (wst.scanned_blocks, wst.scanned_docs, wst.probes, wst.hits)
        # a batch with fewer bins than ranks
        for c in ctxs:
            c.set_option("shard_wg", 2)
        got, st = sh.search_batch(queries[:5], fpx.SearchOptions(500, 3, 10))
        assert got == [full.osnap.search(q, 500, 3, 10) for q in queries[:5]] and st.path_flags & WALKED
    finally:
        sh.snapshot.release()
        full.reader.snapshot.release()
        for g in [g for row in slices for g in row] + full.gpu_segs:
            g.release()
        for c in ctxs:
            c.trim()


# ---- the option ------------------------------------------------------------------------------------------------------------------

def test_the_option_round_trips(env, monkeypatch):
    fpx, ctx = env[0], env[3]
    monkeypatch.delenv("FPX_SHARD_WG", raising=False)
    assert ctx.get_option("shard_wg") == 0                            # the default
    for v in (0, 1, 2):
        ctx.set_option("shard_wg", v)
        assert ctx.get_option("shard_wg") == v
    with pytest.raises(Exception):
        ctx.set_option("shard_wg", 3)
    assert ctx.get_option("shard_wg") == 2                            # a refused value changes nothing
    monkeypatch.setenv("FPX_SHARD_WG", "1")
    ctx.set_option("shard_wg", -1)
    assert ctx.get_option("shard_wg") == 1                            # back to the fallback: the environment, read per call
    monkeypatch.delenv("FPX_SHARD_WG")
    assert ctx.get_option("shard_wg") == 0
