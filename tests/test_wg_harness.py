"""wg_harness.py's makers give, for a fixed seed, the bytes they gave when every suite had a copy of its own: the digests below were
recorded from the copies in test_gpu_side_wg.py, test_gpu_words_wg.py, test_gpu_low_wg.py and test_gpu_low_wg_filtered.py (which agreed
with each other; the side file's _rand_items(rng, first, per, ...) with what the others gave for np.arange(first, first + per)) before
they were removed.  A world or a query of a suite is these makers' output in the order the suite calls them, so a change in the order,
the shape or the dtype of a draw from `rng` shows here, without a GPU.  Then growth() and figures() on hand-made values."""
import hashlib
import types

import numpy as np

import wg_harness as wg

SHARED = 0x2BADF00D
IDS = np.arange(1, 51)                       # 50 docs x 8 hashes
EXTRA = [(SHARED, IDS[:3]), (7, IDS[10:12])]


def _digest(a):
    return hashlib.sha256(f"{a.dtype} {a.shape} ".encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


def _items():
    return wg.rand_items(np.random.default_rng(11), IDS, 8, EXTRA)


def test_rand_items():
    assert _digest(_items()) == "fac50d25e2d8aea2004907122063073a533fcd5846cc8f6299aa7e8469c1d4d2"
    assert _digest(wg.rand_items(np.random.default_rng(11), np.arange(1, 1 + 50), 8, EXTRA, lo=0, hi=1 << 32)) == _digest(_items())
    assert _digest(wg.rand_items(np.random.default_rng(13), IDS, 8)) == "d76f77fa85ffc5f32d99140978af68dcb54af4bd6f5a63cf79780ed31f714646"
    # the words file's range, by name and by its partial's defaults
    words = "29c005dd1637a7d8731406b9caf641c10f20604f094eed169799095fdab479d7"
    assert (wg.WORDS_LO, wg.WORDS_HI) == (0x10000000, 0xF0000000)
    assert _digest(wg.rand_items(np.random.default_rng(12), IDS, 8, EXTRA, lo=wg.WORDS_LO, hi=wg.WORDS_HI)) == words
    assert _digest(wg.rand_items(np.random.default_rng(12), list(IDS), 8, EXTRA, wg.WORDS_LO, wg.WORDS_HI)) == words


def test_aimed():
    items = _items()
    assert _digest(wg.aimed(np.random.default_rng(21), items, 65)) == "07f9e2488bc02df22595537ae2ce6e9c61b0f69a5917d07e9678be8775ee31c2"
    assert _digest(wg.aimed(np.random.default_rng(22), items, 65, [SHARED, 0, 0xFFFFFFFF])) == "428fd56b0b30ad732fedfae4606fffcebfdc25bf440fc540810f7546aea3460a"
    # (a query shorter than its doc's hashes and `extra`: no noise is drawn)
    assert _digest(wg.aimed(np.random.default_rng(23), items, 6, [SHARED])) == "acec19761d6a482ea0892e3df59ab3e282499b1f0cf2111d5c2787df0b973720"
    q = wg.aimed(np.random.default_rng(24), items, 65, [SHARED], 0x10000000, 0xF0000000)
    assert _digest(q) == "dcbd27d0df0cfa42d7ae19b1083d202da111bb6a1c2d22e5422d04c2fc89aab8"
    assert len(q) == 65 and q.dtype == np.uint32 and SHARED in q


def test_sampled_noise_rows_and_post():
    items = _items()
    assert _digest(wg.sampled(np.random.default_rng(31), items, 20)) == "f7f95cfc2835056903caf72d8aecbc7f92855adb33aaf3ed2cbff74f4f40bc43"
    assert _digest(wg.noise(np.random.default_rng(32), 33)) == "c1c8928b61aec33daadc8a89480b2a0407c095ee619851eb04fc32c965f10cc2"
    assert _digest(wg.rows(items, 7)) == "8f2bd29866dc494093f74ff58e5865c5aa9da891b778a1108a514dd785622aac"
    assert _digest(wg.post(SHARED, IDS[:5])) == "b285ceb13b0d8515ccb0dbf15b072d48bbc8f144524d48ae1989582ff717379a"
    assert SHARED in wg.rows(items, 2) and SHARED not in wg.rows(items, 4)


def test_usual():
    assert [(h, list(d)) for h, d in wg.usual(5, 6)(2, IDS)] == [(5, [1, 2, 3, 4]), (6, [1, 2])]
    assert [len(wg.usual(5, 6)(s, np.arange(100))[0][1]) for s in range(5)] == [2, 3, 4, 70, 2]


def test_growth():
    a = {"blocks": [1, 2, 3], "queries": 10}
    b = {"blocks": [1, 5, 3], "queries": 14}
    assert wg.growth(a, b) == {"blocks": [0, 3, 0], "queries": 4}
    assert wg.growth(a, a) == {"blocks": [0, 0, 0], "queries": 0}


def test_figures():
    s = types.SimpleNamespace(hits=4, algorithmic_bytes=5, scanned_docs=2, probes=3, scanned_blocks=1, path_flags=64)
    assert wg.figures(s) == (1, 2, 3, 4, 5)
    assert wg.STATS == ("scanned_blocks", "scanned_docs", "probes", "hits", "algorithmic_bytes")
    assert wg.figures(s) == tuple(getattr(s, f) for f in wg.STATS)
    assert wg.figures(s)[:wg.FOUR] == (1, 2, 3, 4) and wg.figures(s)[:wg.WITH_BYTES] == wg.figures(s)
