"""Index views without a GPU: the host statement of mask -> rows that the GPU tests compare the device with, against
hand-worked masks, and the argument checks that never reach the library."""
import numpy as np
import pytest


def test_pack_mask_hand_worked():
    from gulon_amd.index import pack_mask
    keep = np.zeros(130, bool)
    keep[[0, 2, 63, 64, 127, 129]] = True
    assert pack_mask(keep, 130).tolist() == [(1 << 0) | (1 << 2) | (1 << 63), (1 << 0) | (1 << 63), 1 << 1]
    assert pack_mask(np.ones(64, bool), 64).tolist() == [2 ** 64 - 1]
    assert pack_mask(np.ones(65, bool), 65).tolist() == [2 ** 64 - 1, 1]
    assert pack_mask(np.array([False, True, True]), 3).tolist() == [6]
    words = np.array([5, 9], np.uint64)
    assert pack_mask(words, 100) is not None and pack_mask(words, 100).tolist() == [5, 9]
    assert pack_mask(words.view(np.int64), 128).dtype == np.uint64
    for bad, n in ((np.ones(5, bool), 6), (words, 129), (words, 64), (np.ones(2, np.int32), 100)):
        with pytest.raises(ValueError):
            pack_mask(bad, n)


def test_mask_rows_hand_worked():
    from gulon_amd.index import mask_rows, pack_mask
    assert mask_rows(np.array([0b1011], np.uint64), 64).tolist() == [0, 1, 3]
    assert mask_rows(np.array([0b1011], np.uint64), 2).tolist() == [0, 1]          # bits at and above n are ignored
    assert mask_rows(np.array([1 << 63, 1, 2 ** 64 - 1], np.uint64), 131).tolist() == [63, 64, 128, 129, 130]
    assert mask_rows(np.array([2 ** 64 - 1], np.uint64), 1).tolist() == [0]
    assert mask_rows(np.zeros(3, np.uint64), 150).tolist() == []
    assert mask_rows(np.zeros(1, np.uint64), 0).tolist() == []
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 1000, 64 * 64 * 3 + 5):
        keep = rng.random(n) < 0.3
        assert mask_rows(pack_mask(keep, n), n).tolist() == np.flatnonzero(keep).tolist()


def test_package_exports_the_view():
    import gulon_amd as g
    assert issubclass(g.PQIndexView, g.PQIndex)
    for name in ("select", "batch_query_raw", "positions_raw", "rows", "map_positions", "context"):
        assert hasattr(g.PQIndexView, name), name
    assert callable(g.PQIndex.select) and callable(g.SortedIndex.select) and callable(g.WordIndex.restrict)


def test_cli_parses_restrict():
    from gulon_amd import cli
    p = cli._parser()
    assert p.parse_args(["query-words", "-i", "x", "-r", "words.txt"]).restrict == "words.txt"
    assert p.parse_args(["query", "-i", "x", "--restrict", "w", "q.vec"]).restrict == "w"
    assert p.parse_args(["query-words", "-i", "x"]).restrict is None
    for argv in (["query-words", "-i", "x", "-r", "w", "-v", "vec"], ["query-words", "-i", "x", "-r", "w", "-x"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
