"""Word-pair similarity on the device (csrc/pairs.hip, gulon_amd/similarity.py): the pair distances of every handle form
and the rank sums, bit for bit against the numpy references; the device route against the generic route; the command end
to end; a handle used for pair distances against a fresh one."""
import io

import numpy as np
import pytest

import handle_history as hh
from conftest import bits

pytestmark = pytest.mark.gpu

N_ROWS = 200                                   # four 64-row blocks, the last one ragged
PAIR_COUNTS = (1, 64, 65, 130)                 # one lane; a full wave; a wave and one lane; two waves and two lanes


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


def _fixed(n_rows):
    """a == b (twice: inside a block and on the last row); both rows in one block; the first and the last row, both ways"""
    last = n_rows - 1
    return [(5, 5), (3, 40), (0, last), (last, 0), (last, last)]


def _pairs(count, n_rows, seed):
    rng = np.random.default_rng([seed, count, n_rows])
    a, b = rng.integers(0, n_rows, count).astype(np.int32), rng.integers(0, n_rows, count).astype(np.int32)
    if count >= 10:                                            # the fixed pairs at the head and at the ragged tail
        for i, (x, y) in enumerate(_fixed(n_rows)):
            a[i], b[i] = x, y
            a[count - 1 - i], b[count - 1 - i] = y, x
    return a, b


def _dev(fn, a, b):
    """a *_pair_distances_dev method on torch's buffers"""
    import torch
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((len(a),), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fn(ta.data_ptr(), tb.data_ptr(), len(a), out.data_ptr())
    return out.cpu().numpy()


def _check_pairs(index, lookup, n_rows, seed):
    """Both forms of index.pair_distances at every pair count against distanceSq(lookup(a), lookup(b)); a == b gives +0;
    a row outside [0, n_rows) is an error in both forms, wherever it stands."""
    from gulon_amd.similarity import pair_distance_reference
    cases = [_pairs(count, n_rows, seed) for count in PAIR_COUNTS if count > 1]
    cases += [(np.array([x], np.int32), np.array([y], np.int32)) for x, y in _fixed(n_rows)]      # count 1
    for a, b in cases:
        want = pair_distance_reference(lookup(a), lookup(b))
        assert np.array_equal(bits(want)[a == b], np.zeros(int((a == b).sum()), np.uint32))
        got = index.pair_distances(a, b)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(_dev(index.pair_distances_dev, a, b)), bits(want))
    assert any(len(a) == 130 and (a == b).any() and (a != b).any() for a, b in cases)
    a, b = _pairs(65, n_rows, seed)
    for at, value, side in ((64, n_rows, 0), (0, -1, 1), (33, 2 ** 31 - 1, 1)):
        bad = [a.copy(), b.copy()]
        bad[side][at] = value
        with pytest.raises(ValueError, match=rf"pair {at} = "):
            index.pair_distances(*bad)
        with pytest.raises(ValueError, match="outside"):
            _dev(index.pair_distances_dev, *bad)
    assert len(index.pair_distances([], [])) == 0
    index.pair_distances_dev(None, None, 0, None)               # n == 0: nothing is touched
    assert np.array_equal(bits(index.pair_distances(a, b)), bits(pair_distance_reference(lookup(a), lookup(b))))


def _codes(g, d, m, k, seed, n=N_ROWS):
    rng = np.random.default_rng([seed, d, m, k])
    cents = rng.standard_normal(k * d).astype(np.float32)
    idx = rng.integers(0, k, (m, n)).astype(np.int32)
    pq = g.ProductQuantizer.from_flat(k, d, m, cents)
    coder = pq.coder_factory(n)
    return pq, g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(m)])


# d, m, k: uneven sub-vectors 4/3/3 with 4-bit codes; two 16-byte code words; wide codes
FLAT = {"4bit": (10, 3, 16), "two_words": (40, 20, 256), "wide": (12, 4, 1024)}


@pytest.mark.parametrize("form", list(FLAT))
def test_flat_index_pair_distances(g, form):
    d, m, k = FLAT[form]
    ix = g.PQIndex(*_codes(g, d, m, k, 1))
    try:
        _check_pairs(ix, ix.decode_rows, N_ROWS, 11)
        sx = g.SortedIndex(ix, "cosine")                        # the rows as stored, whatever the metric
        a, b = _pairs(64, N_ROWS, 12)
        assert np.array_equal(bits(sx.pair_distances(a, b)), bits(ix.pair_distances(a, b)))
    finally:
        ix.close()


@pytest.mark.parametrize("form", ["two_words", "wide"])
def test_view_pair_distances_are_over_its_positions(g, form):
    d, m, k = FLAT[form]
    ix = g.PQIndex(*_codes(g, d, m, k, 2))
    view = ix.select(rows=np.arange(1, N_ROWS, 3))             # 67 rows: a row id 67 is the root's, not the view's
    try:
        assert view.length == 67
        _check_pairs(view, view.decode_rows, 67, 13)
        a, b = _pairs(65, 67, 14)
        assert np.array_equal(bits(view.pair_distances(a, b)), bits(ix.pair_distances(view.rows[a], view.rows[b])))
    finally:
        view.close()
        ix.close()


def test_grouped_index_pair_distances_use_the_lookup_partition(g):
    """offsets 50, 50, 50, 120: groups 1 and 2 are empty, and for row 50 Arrays.binarySearch lands on the middle 50 -- the
    partition of lookup is group 2, while the row's own group (the one a query scans it in) is group 3."""
    from gulon_amd.similarity import pair_distance_reference
    d, m, k = 10, 3, 16
    pq, enc = _codes(g, d, m, k, 3)
    centroids = np.random.default_rng(4).standard_normal((5, d)).astype(np.float32)
    gx = g.GroupedIndex(pq, enc, centroids, [50, 50, 50, 120], g.LimitGroups(2))
    flat = g.PQIndex(pq, enc)
    try:
        residual = flat.decode_rows([50])[0]
        assert np.array_equal(bits(gx.lookup_rows([50])[0]), bits(centroids[2] + residual))
        assert not np.array_equal(centroids[2] + residual, centroids[3] + residual)
        _check_pairs(gx, gx.lookup_rows, N_ROWS, 15)
        a = np.array([50, 50, 49, 50, 119, 120], np.int32)      # row 50 against rows of groups 0, 3 and 4, and itself
        b = np.array([49, 51, 50, 50, 120, 50], np.int32)
        want = pair_distance_reference(gx.lookup_rows(a), gx.lookup_rows(b))
        assert np.array_equal(bits(gx.pair_distances(a, b)), bits(want))
        own = pair_distance_reference((centroids[3] + residual)[None, :], gx.lookup_rows([51]))
        assert bits(want)[1] != bits(own)[0]                    # the row's own group would have given another distance
    finally:
        flat.close()
        gx.close()


@pytest.mark.parametrize("d", [7, 33, 40, 128])
def test_dataset_pair_distances(g, d):
    """d = 7: no 16-byte row load; 33 and 40: across a tile step of 32 coordinates, without and with 16-byte loads; 128."""
    X = np.random.default_rng([5, d]).standard_normal((N_ROWS, d)).astype(np.float32)
    dm = g.DeviceMatrix.from_host(X)
    ex = g.ExactIndex(dm, "l2", 10, 150)                       # the rows are the matrix's, whatever the index's range
    try:
        _check_pairs(ex, lambda rows: X[np.asarray(rows, np.int64)], N_ROWS, 16)
    finally:
        ex.close()
        dm.close()


# ---- rank sums -----------------------------------------------------------------------------------------------------------

def _scores(n, seed):
    """Heavy ties (six and eleven distinct values), +inf twice, -0 beside +0, one NaN x, interleaved sections 0..2, one
    section id above and one below the range."""
    rng = np.random.default_rng([seed, n])
    x = rng.integers(0, 6, n).astype(np.float32)
    y = rng.integers(0, 11, n).astype(np.float32)
    section = rng.integers(0, 3, n).astype(np.int32)
    if n >= 256:
        x[[3, 200]] = np.inf
        x[[4, 100, 201]] = [-0.0, 0.0, -0.0]
        y[[5, 6]] = [-0.0, 0.0]
        x[7] = np.nan
        y[8] = np.nan
        section[[3, 200, 4, 100, 201]] = 1                      # the infinities and the zeros meet in one section
        section[9], section[n - 1] = 3, -1
    return x, y, section


@pytest.mark.parametrize("n", [1, 2, 256, 257, 600])
def test_rank_sums_against_numpy(g, n):
    import torch
    from gulon_amd.similarity import rank_sums, rank_sums_reference
    N = g.native
    x, y, section = _scores(n, 21)
    want = rank_sums_reference(x, y, section, 3)
    pooled = rank_sums_reference(x, y, None, 1)
    if n >= 256:
        assert want[:, 4].sum() == 2 and want[:, 0].sum() == n - 4 and pooled[0, 0] == n - 2 and pooled[0, 4] == 2
    got = rank_sums(x, y, section, 3)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(rank_sums(x, y), pooled)              # section = NULL
    tx, ty, ts = (torch.from_numpy(v).cuda() for v in (x, y, section))
    out = torch.full((4, 5), 99, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib().gulon_rank_sums_dev(tx.data_ptr(), ty.data_ptr(), ts.data_ptr(), n, 3, out.data_ptr(), None))
    N.check(N.lib().gulon_rank_sums_dev(tx.data_ptr(), ty.data_ptr(), None, n, 1, out[3].data_ptr(), None))
    N.check(N.lib().gulon_device_synchronize())
    assert np.array_equal(out.cpu().numpy(), np.concatenate([want, pooled]))


def test_rank_sums_of_nothing_and_bad_arguments(g):
    from gulon_amd.similarity import rank_sums
    assert not rank_sums([], [], [], 4).any() and rank_sums([], [], [], 4).shape == (4, 5)
    with pytest.raises(ValueError, match="expected 1 section"):
        rank_sums([1.0], [1.0], None, 2)
    with pytest.raises(ValueError, match="at least 1"):
        rank_sums([1.0], [1.0], [0], 0)


# ---- the routes ------------------------------------------------------------------------------------------------------------

N_WORDS, D = 600, 16
WORDS = [f"w{i:04d}" for i in range(N_WORDS)]            # String order = row order


@pytest.fixture(scope="module")
def indexes(g):
    """A sorted and a grouped WordIndex over the same words, and the true vectors."""
    from gulon_amd.grouped import GroupedIndex, group
    from gulon_amd.kmeans import Config as KMeansConfig
    X = np.random.default_rng(31).standard_normal((N_WORDS, D)).astype(np.float32)
    dm = g.DeviceMatrix.from_host(X)
    pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(32, 4, 3))
    sorted_index = g.WordIndex(WORDS, g.Index.sorted(dm, pq, "l2"))
    clustering = g.KMeans.compute_clusters(g.Vectors(dm), KMeansConfig(6, 3))
    gv = group(dm, clustering)
    rpq = g.ProductQuantizer.apply(gv.residuals, g.ProductQuantizerConfig(32, 4, 3))
    gx = GroupedIndex(rpq, rpq.encode(gv.residuals), gv.centroids, gv.offsets, g.LimitGroups(3), "l2")
    grouped_index = g.WordIndex([WORDS[i] for i in gv.perm], gx)
    exact = g.ExactWordIndex(WORDS, g.ExactIndex(dm, "l2"))
    return {"sorted": sorted_index, "grouped": grouped_index, "exact": exact, "X": X}


def _sections(X):
    """monotone: the score is the negated true distance; noisy: a coarse score with many ties; a section without a
    header name; absent words; an empty section."""
    from gulon_amd.similarity import pair_distance_reference
    rng = np.random.default_rng(32)
    rows = rng.integers(0, N_WORDS, (300, 2))
    dist = pair_distance_reference(X[rows[:, 0]], X[rows[:, 1]])
    monotone = [(WORDS[a], WORDS[b], -float(v)) for (a, b), v in zip(rows[:120], dist[:120])]
    noisy = [(WORDS[a], WORDS[b], float(np.round(10 - v / 4 + rng.normal()))) for (a, b), v in zip(rows[120:], dist[120:])]
    odd = [("w0001", "absent", 1.0), ("absent", "w0002", 2.0), ("W0003", "w0004", 3.0), ("w0005", "w0005", 9.0),
           ("w0006", "w0007", 2.0), ("w0008", "w0009", 2.0)]
    return [("monotone", monotone), ("noisy", noisy[:90]), ("", noisy[90:]), ("odd", odd), ("empty", [])]


@pytest.mark.parametrize("kind", ["sorted", "grouped", "exact"])
def test_the_routes_give_one_report(g, indexes, kind):
    from gulon_amd.similarity import evaluate_pairs, pair_distance_reference, rank_sums_reference, spearman
    target, sections = indexes[kind], _sections(indexes["X"])
    device = evaluate_pairs(target, sections)
    generic = evaluate_pairs(target, sections, route="generic")
    assert device == generic and device.lines() == generic.lines()
    by_name = {s.name: s for s in device.sections}
    assert [(s.name, s.n, s.skipped, s.dropped) for s in device.sections] == \
        [("monotone", 120, 0, 0), ("noisy", 90, 0, 0), ("", 90, 0, 0), ("odd", 3, 3, 0), ("empty", 0, 0, 0)]
    assert (device.total.n, device.total.skipped) == (303, 3) and np.isnan(by_name["empty"].rho)
    assert device.lines()[4] == "empty: rho nan (n = 0, skipped 0, dropped 0)"
    # the sums, from the vectors `lookup` hands out
    live = [(a, b, s) for _, pairs in sections for a, b, s in pairs
            if target.row_of(a) is not None and target.row_of(b) is not None]
    x = pair_distance_reference(np.stack([target.lookup(a) for a, _, _ in live]),
                                np.stack([target.lookup(b) for _, b, _ in live]))
    sums = rank_sums_reference(x, np.float32([s for _, _, s in live]), None, 1)[0]
    assert (device.total.sxy, device.total.sxx, device.total.syy) == tuple(int(v) for v in sums[1:4])
    assert device.total.rho == 0.0 - spearman(*sums[1:4])
    # the report negates: the scores fall as the true distance grows, and an index's distances grow with the true ones
    assert by_name["noisy"].rho > 0
    if kind == "exact":
        assert by_name["monotone"].rho == 1.0 and device.lines()[0] == "monotone: rho 1.0000 (n = 120, skipped 0, dropped 0)"
        # noisy: score = round(10 - dist / 4 + N(0, 1)); dist / 4 has standard deviation 2 * sqrt(2 * 16) / 4 = 2.8 against
        # 1.04 of the noise and the rounding, a Pearson correlation of 0.94
        assert by_name["noisy"].rho > 0.8
    assert target.distances([("w0005", "w0005"), ("w0001", "absent"), ("w0006", "w0007")])[:2] == [np.float32(0), None]
    want = pair_distance_reference(target.lookup("w0006"), target.lookup("w0007"))
    assert bits(target.distances([("w0006", "w0007")])[0]) == bits(want)


def test_the_command_end_to_end(g, indexes, tmp_path):
    from gulon_amd import cli
    from gulon_amd.index_file import dump_index
    from gulon_amd.similarity import evaluate_pairs, read_pairs
    X = indexes["X"]
    index_path, vectors_path, pairs_path = (str(tmp_path / n) for n in ("words.idx", "vectors.txt", "pairs.txt"))
    with open(index_path, "wb") as fh:
        fh.write(dump_index(indexes["sorted"].index, WORDS))
    with open(vectors_path, "w") as fh:
        fh.write(f"{N_WORDS} {D}\n")
        for w, row in zip(WORDS, X):
            fh.write(w + " " + " ".join(repr(float(x)) for x in row) + "\n")
    sections = _sections(X)
    text = "# two benchmarks in one file\n\n"
    for name, pairs in sections[:2]:
        text += f": {name}\n" + "".join(f"{a.upper()}\t{b.upper()} {s!r}\n" for a, b, s in pairs)
    text += ": odd\nw0001 absent 1.0\n"
    with open(pairs_path, "w") as fh:
        fh.write(text)
    read = read_pairs(text.splitlines(), lowercase=True)
    assert [name for name, _ in read] == ["monotone", "noisy", "odd"]

    def run(extra):
        out = io.BytesIO()
        assert cli.main(["similarity", "-i", index_path, "--lowercase"] + extra + [pairs_path], stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()
    lines = run([])
    assert lines == evaluate_pairs(indexes["sorted"], read).lines()
    assert len(lines) == 4 and lines[3].startswith("total: rho ") and lines[2] == "odd: rho nan (n = 0, skipped 1, dropped 0)"
    exact = run(["-v", vectors_path, "--exact"])
    assert exact == evaluate_pairs(indexes["exact"], read).lines()
    assert exact[0] == "monotone: rho 1.0000 (n = 120, skipped 0, dropped 0)" and exact != lines
    out = io.BytesIO()                                       # without --lowercase no upper-case word is found
    assert cli.main(["similarity", "-i", index_path, pairs_path], stdout=out) == 0
    assert out.getvalue().decode("utf-8").splitlines()[0] == "monotone: rho nan (n = 0, skipped 120, dropped 0)"


# ---- a used handle -----------------------------------------------------------------------------------------------------------

def test_a_handle_used_for_pair_distances_answers_like_a_fresh_one(g, oracle):
    w = hh.world("m16")
    pq = g.ProductQuantizer.from_flat(w.k, w.d, w.m, w.cents)
    coder = pq.coder_factory(w.n)
    parts = (pq, g.EncodedMatrix(coder, [coder.build_code(w.idx[j]) for j in range(w.m)]))
    used, fresh = g.PQIndex(*parts), g.PQIndex(*parts)
    try:
        a, b = _pairs(130, w.n, 41)
        first = used.pair_distances(a, b)
        assert np.array_equal(bits(_dev(used.pair_distances_dev, a, b)), bits(first))
        with pytest.raises(ValueError):
            used.pair_distances([0, w.n], [0, 0])
        for call in hh.probes(w):
            Q = hh.queries(oracle, w, call)
            got = used.batch_query_raw(call.K, Q, call.frm, call.until)
            hh.same_answer(got, hh.expected(oracle, w, call))
            hh.same_as_fresh(got, fresh.batch_query_raw(call.K, Q, call.frm, call.until), hh.expected(oracle, w, call))
        assert np.array_equal(bits(used.pair_distances(a, b)), bits(first))
    finally:
        used.close()
        fresh.close()
