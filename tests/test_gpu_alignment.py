"""Alignment on the device (csrc/alignment.hip, gulon_amd/alignment.py): the pair moment bit for bit against
its numpy restatement and against the full-matrix moment, the mutual test, the argument checks, the seed solve, the
refinement loop against the float64 restatement of tests/alignment_ref.py, and the two commands on files."""
import functools
import io

import numpy as np
import pytest

import alignment_ref as ref
import gulon_amd as g
from gulon_amd import alignment, cli, rotation
from gulon_amd import native as N
from gulon_amd.refine import _DeviceArray

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 9001)
ROWS_A, ROWS_B = 700, 500                      # the two matrices differ in rows as well as in dimension


def same64(got, want):
    """NaN in the same places, the same bits everywhere else."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def spread(rng, n, d):
    """Mixed signs, magnitudes spread over 2^-20 .. 2^20: sums whose bits depend on the order of the additions."""
    return (rng.choice([-1.0, 1.0], (n, d)) * 2.0 ** rng.uniform(-20, 20, (n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def matrices(da, db, wide=False):
    rng = np.random.default_rng([da, db, int(wide)])
    if wide:
        a, b = spread(rng, ROWS_A, da), spread(rng, ROWS_B, db)
    else:
        a, b = rng.normal(size=(ROWS_A, da)).astype(np.float32), rng.normal(size=(ROWS_B, db)).astype(np.float32)
    return a, b, g.DeviceMatrix.from_host(a), g.DeviceMatrix.from_host(b)


def pair_lists(n, seed):
    """Shuffled, with duplicates (n may exceed the rows), about one row in ten negative on either side."""
    rng = np.random.default_rng([seed, n])
    ra, rb = rng.integers(0, ROWS_A, n), rng.integers(0, ROWS_B, n)
    ra[rng.random(n) < 0.1] = -1
    rb[rng.random(n) < 0.1] = rng.integers(-9, 0)
    return ra.astype(np.int32), rb.astype(np.int32)


def moment_dev(A, B, ra, rb):
    """gulon_dataset_pair_moment_dev on lists this test uploads."""
    da, db = _DeviceArray(), _DeviceArray()
    try:
        if len(ra):
            da.upload(ra), db.upload(rb)
        return alignment.pair_moment_dev(A, B, da.ptr if len(ra) else None, db.ptr if len(ra) else None, len(ra))
    finally:
        da.free(), db.free()


# ---- 1. the pair moment --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("da,db", [(1, 1), (24, 24), (65, 100), (300, 300)])
def test_pair_moment_bit_for_bit(da, db, n):
    a, b, A, B = matrices(da, db)
    ra, rb = pair_lists(n, da)
    want, used = alignment.pair_moment_reference(a, b, ra, rb)
    got, got_used = alignment.pair_moment(A, B, ra, rb)
    assert got_used == used == int(((ra >= 0) & (rb >= 0)).sum())
    same64(got, want)
    dev, dev_used = moment_dev(A, B, ra, rb)                      # the device-pointer form: the same bits, the same count
    assert dev_used == used
    same64(dev, want)
    again, _ = alignment.pair_moment(A, B, ra, rb)                # and the same bits on a second call
    same64(again, got)
    if n == 0:
        assert used == 0 and not got.any()


def test_pair_moment_keeps_the_order_where_the_order_shows():
    a, b, A, B = matrices(24, 24, wide=True)
    ra, rb = pair_lists(9001, 7)
    want, used = alignment.pair_moment_reference(a, b, ra, rb)
    backwards, _ = alignment.pair_moment_reference(a, b, ra[::-1], rb[::-1])
    assert not np.array_equal(want, backwards)                   # the inputs do tell one order from another
    got, got_used = alignment.pair_moment(A, B, ra, rb)
    assert got_used == used
    same64(got, want)
    same64(moment_dev(A, B, ra, rb)[0], want)
    same64(alignment.pair_moment(A, B, ra[::-1].copy(), rb[::-1].copy())[0], backwards)


@pytest.mark.parametrize("n,da,db", [(1, 1, 1), (4097, 65, 100), (9001, 24, 24)])
def test_identity_lists_give_the_full_matrix_moment(n, da, db):
    rng = np.random.default_rng([n, da, db])
    a, b = spread(rng, n, da), spread(rng, n, db)
    A, B = g.DeviceMatrix.from_host(a), g.DeviceMatrix.from_host(b)
    rows = np.arange(n, dtype=np.int32)
    full = rotation.moment(A, B)
    got, used = alignment.pair_moment(A, B, rows, rows)
    assert used == n
    same64(got, full)
    same64(moment_dev(A, B, rows, rows)[0], full)
    same64(alignment.pair_moment_reference(a, b, rows, rows)[0], full)
    A.close(), B.close()


# ---- 2. mutual rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", (1, 255, 256, 257, 70001))
def test_mutual_rows_match_the_reference(ns):
    nt = ns + 37 if ns % 2 else max(ns - 19, 1)
    rng = np.random.default_rng([ns, nt])
    fwd = rng.integers(0, nt, ns).astype(np.int32)
    bwd = rng.integers(0, ns, nt).astype(np.int32)
    agree = rng.random(ns) < 0.5                                  # half of the rows are chosen back
    bwd[fwd[agree]] = np.flatnonzero(agree)                        # (a target row asked twice keeps the last)
    fwd[rng.random(ns) < 0.1] = -1
    fwd[rng.random(ns) < 0.1] = nt + rng.integers(0, 5)
    if ns > 1:
        fwd[0], fwd[1] = nt, np.iinfo(np.int32).max
    want = alignment.mutual_rows_reference(fwd, bwd)
    assert ns == 1 or (want >= 0).any()
    assert np.array_equal(alignment.mutual_rows(fwd, bwd), want)
    dev = {name: _DeviceArray() for name in ("fwd", "bwd", "out")}
    try:
        dev["fwd"].upload(fwd), dev["bwd"].upload(bwd), dev["out"].ensure(4 * ns)
        N.check(N.lib().gulon_mutual_rows_dev(dev["fwd"].ptr, ns, dev["bwd"].ptr, nt, dev["out"].ptr, None))
        N.check(N.lib().gulon_device_synchronize())
        assert np.array_equal(dev["out"].download(np.zeros(ns, np.int32)), want)
    finally:
        for a in dev.values():
            a.free()


# ---- 3. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors():
    import ctypes as C
    L = N.lib()
    _, _, A, B = matrices(24, 24)
    out, used = np.zeros(24 * 24), C.c_int64(-5)
    rows = np.zeros(4, np.int32)
    p = rows.ctypes.data
    for fn in (L.gulon_dataset_pair_moment, L.gulon_dataset_pair_moment_dev):
        assert fn(None, B._h, p, p, 4, out, C.byref(used)) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, None, p, p, 4, out, C.byref(used)) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, B._h, None, p, 4, out, C.byref(used)) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, B._h, p, None, 4, out, C.byref(used)) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, B._h, p, p, 4, out, None) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, B._h, p, p, -1, out, C.byref(used)) == N.ERR_INVALID_ARGUMENT
        assert fn(A._h, B._h, None, None, 0, out, C.byref(used)) == N.OK and used.value == 0    # no pairs: no lists
    for ra, rb in (([0, ROWS_A], [0, 0]), ([0, 0], [ROWS_B, 0]), ([-1, 0], [ROWS_B, 0])):
        with pytest.raises(ValueError, match="beyond"):
            alignment.pair_moment(A, B, ra, rb)                    # the host form names the pair
    alignment.pair_moment(A, B, [ROWS_A - 1, -1], [ROWS_B - 1, -(2 ** 31)])                       # the last rows are rows
    with pytest.raises(ValueError, match="2 rows of a for 1 rows of b"):
        alignment.pair_moment(A, B, [0, 1], [0])
    for fn in (L.gulon_mutual_rows, L.gulon_mutual_rows_dev):
        extra = (None,) if fn is L.gulon_mutual_rows_dev else ()
        assert fn(None, 4, p, 4, p, *extra) == N.ERR_INVALID_ARGUMENT
        assert fn(p, 4, None, 4, p, *extra) == N.ERR_INVALID_ARGUMENT
        assert fn(p, 4, p, 4, None, *extra) == N.ERR_INVALID_ARGUMENT
        assert fn(p, -1, p, 4, p, *extra) == N.ERR_INVALID_ARGUMENT
        assert fn(p, 4, p, -1, p, *extra) == N.ERR_INVALID_ARGUMENT
        assert fn(None, 0, None, 0, None, *extra) == N.OK
    assert alignment.mutual_rows([0, 3], []).tolist() == [-1, -1]                               # no target rows at all


# ---- 4. the seed ---------------------------------------------------------------------------------------------------------------
def vectors_of(words, x):
    return g.DeviceWordVectors(words, g.DeviceMatrix.from_host(x))


def test_seed_alignment_recovers_an_exact_map():
    rng = np.random.default_rng(24)
    n, d = 50, 24
    y = ref.unit(rng.normal(size=(n, d))).astype(np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    perm = rng.permutation(n)
    x = (y[perm].astype(np.float64) @ q.T).astype(np.float32)       # X Q = Y[perm] up to the rounding of X
    source, target = vectors_of([f"s{i}" for i in range(n)], x), vectors_of([f"t{i}" for i in range(n)], y)
    pairs = [(f"s{i}", f"t{perm[i]}") for i in rng.choice(n, 30, replace=False)]
    pairs[3:3] = [("nowhere", "t1"), ("s1", "nothing")]
    rot, used, skipped = alignment.seed_alignment(source, target, pairs)
    assert (used, skipped) == (30, 2) and rot.dimension == d
    assert rot.orthogonality_error() <= 2.0 ** -22               # the bound of test_gpu_rotation's Procrustes step
    mapped = rot.apply(x).astype(np.float64)
    error = float(((mapped - y[perm]) ** 2).sum())
    slack = 4 * d ** 1.5 * 2.0 ** -24 * float((x.astype(np.float64) ** 2).sum())      # that test's slack on a squared error
    print(f"|X W - Y[perm]|^2 = {error:.3e} (slack {slack:.3e}), |W - Q| = {np.abs(rot.matrix - q).max():.3e}")
    assert error <= slack
    with pytest.raises(ValueError, match="none of the 1 dictionary pairs"):
        alignment.seed_alignment(source, target, [("s1", "s1")])
    source.matrix.close(), target.matrix.close()


# ---- 5. refinement, end to end -------------------------------------------------------------------------------------------------
S_WORDS = [f"s{i:03d}" for i in range(ref.N)]
T_WORDS = [f"t{i:03d}" for i in range(ref.N)]


@pytest.fixture(scope="module")
def case():
    x, y, perm, q, rows = ref.fixture(1)
    out = {"x": x, "y": y, "perm": perm, "source": vectors_of(S_WORDS, x), "target": vectors_of(T_WORDS, y),
           "seed": [(S_WORDS[s], T_WORDS[t]) for s, t in rows], "seed_rows": rows,
           "gold": [(S_WORDS[i], T_WORDS[perm[i]]) for i in range(ref.N)]}
    yield out
    out["source"].matrix.close(), out["target"].matrix.close()


def precision_at_1(case, rot):
    """evaluate_dictionary by plain nearest neighbours, on exact indexes over the mapped source and the target."""
    mapped = rot.apply_device(case["source"].matrix)
    source = g.ExactWordIndex(S_WORDS, g.ExactIndex(mapped, "cosine"))
    target = g.ExactWordIndex(T_WORDS, g.ExactIndex(case["target"].matrix, "cosine"))
    try:
        report = g.evaluate_dictionary(target, source, case["gold"], ks=(1,), method="nn")
        assert report.asked == ref.N and report.skipped == 0
        return report.precision(1)
    finally:
        source.close(), target.close(), mapped.close()


def test_refinement_end_to_end(case):
    """A float64 numpy restatement of this pipeline (tests/alignment_ref.py), run on the CPU over generator seeds 1-4,
    gave seed-only P@1 of 0.79-0.89, P@1 of 1.0 from the first round on and 278-317 mutual pairs of 384."""
    lines = []
    rot, history = alignment.train_alignment(case["source"], case["target"], case["seed"], rounds=ref.ROUNDS,
                                             max_rank=ref.MAX_RANK, neighbours=ref.NEIGHBOURS, write=lines.append)
    seed_rot, used, skipped = alignment.seed_alignment(case["source"], case["target"], case["seed"])
    w, chosen, ref_history, _ = ref.train(case["x"], case["y"], case["seed_rows"])
    seed_p1, refined_p1 = precision_at_1(case, seed_rot), precision_at_1(case, rot)
    ref_p1 = ref.precision_at_1(case["x"], case["y"], w, case["perm"])
    print(f"seed-only P@1 {seed_p1:.4f}, refined {refined_p1:.4f} (numpy {ref_p1:.4f}); rounds {history['rounds']}, "
          f"chosen {history['chosen']}; numpy rounds {ref_history}, chosen {chosen}")
    assert history["seed"] == {"used": used, "skipped": skipped} == {"used": ref.SEED_PAIRS, "skipped": 0}
    assert rot.orthogonality_error() <= 2.0 ** -22
    assert refined_p1 >= seed_p1 + 0.05
    assert abs(refined_p1 - ref_p1) <= 2 / ref.N                 # a near-tie allowance, not a tolerance to tune
    assert len(history["rounds"]) == ref.ROUNDS + 1
    for r in history["rounds"]:
        assert 0 < r["mutual"] <= r["asked"] == ref.MAX_RANK
    criteria = [r["criterion"] for r in history["rounds"]]
    assert history["chosen"] == int(np.argmax(criteria))
    # the criterion is a mean cosine: the one of the chosen round, recomputed from the map that came back
    fwd, match = alignment.induce_matches(case["source"].matrix, case["target"].matrix, rot, ref.MAX_RANK, ref.NEIGHBOURS)
    try:
        f, m = (a.download(np.zeros(ref.MAX_RANK, np.int32)) for a in (fwd, match))
        assert f.shape == m.shape == (ref.MAX_RANK,) and ((m == f) | (m == -1)).all() and (f >= 0).all()
        assert int((m >= 0).sum()) == history["rounds"][history["chosen"]]["mutual"]
        cos = np.einsum("ij,ij->i", case["x"][:len(f)].astype(np.float64) @ rot.matrix.astype(np.float64),
                        case["y"][f].astype(np.float64))
        assert abs(cos.mean() - criteria[history["chosen"]]) <= 1e-12
    finally:
        fwd.free(), match.free()
    assert sum("RUNNING" in l for l in lines) == sum("SUCCESS" in l for l in lines) == ref.ROUNDS + 2   # the seed, the rounds


def test_no_rounds_return_the_seed(case):
    """rounds = 0: one induction for the criterion, no solve; the map is the seed's."""
    rot, history = alignment.train_alignment(case["source"], case["target"], case["seed"], rounds=0, max_rank=ref.MAX_RANK)
    assert len(history["rounds"]) == 1 and history["chosen"] == 0
    seed_rot, _, _ = alignment.seed_alignment(case["source"], case["target"], case["seed"])
    assert np.array_equal(rot.matrix, seed_rot.matrix)
    with pytest.raises(ValueError, match="negative"):
        alignment.train_alignment(case["source"], case["target"], case["seed"], rounds=-1)


# ---- 6. the commands on files --------------------------------------------------------------------------------------------------
def write_vectors(path, words, x):
    with open(path, "w") as fh:
        fh.write(f"{len(words)} {x.shape[1]}\n")
        for w, row in zip(words, x):
            fh.write(w + " " + " ".join(repr(float(v)) for v in row) + "\n")


def test_the_commands_on_files(case, tmp_path):
    from gulon_amd.index_file import dump_index
    paths = {n: str(tmp_path / n) for n in ("source.txt", "target.txt", "aligned.txt", "seed.txt", "gold.txt", "en-fr.map",
                                            "target.idx")}
    write_vectors(paths["source.txt"], S_WORDS, case["x"])
    write_vectors(paths["target.txt"], T_WORDS, case["y"])
    for name, pairs in (("seed.txt", case["seed"]), ("gold.txt", case["gold"])):
        with open(paths[name], "w") as fh:
            fh.write("".join(f"{s} {t}\n" for s, t in pairs))
    out = io.BytesIO()
    assert cli.main(["align", "-s", paths["source.txt"], "-t", paths["target.txt"], "-d", paths["seed.txt"], "-o",
                     paths["en-fr.map"], "--rounds", "2", "--max-rank", str(ref.MAX_RANK)], stdout=out) == 0
    lines = out.getvalue().decode("utf-8").splitlines()
    assert len(lines) == 5 and lines[0] == f"seed: {ref.SEED_PAIRS} pairs, skipped 0"
    for t in range(3):
        assert lines[1 + t].startswith(f"round {t}: mutual ") and f" of {ref.MAX_RANK}, criterion 0." in lines[1 + t]
    assert lines[4] in ("chosen: round 0", "chosen: round 1", "chosen: round 2")
    learned = rotation.Rotation.load(paths["en-fr.map"])          # a loadable map
    assert learned.dimension == ref.D and learned.orthogonality_error() <= 2.0 ** -22
    # the file holds what train_alignment returns for the vectors as the command reads them
    source, target = cli.read_ranked(paths["source.txt"]), cli.read_ranked(paths["target.txt"])
    assert source.words == S_WORDS and source.key_index is None    # file order: the row is the rank
    want, history = alignment.train_alignment(source, target, case["seed"], rounds=2, max_rank=ref.MAX_RANK)
    assert np.array_equal(learned.matrix, want.matrix) and lines[4] == f"chosen: round {history['chosen']}"
    assert lines[1] == (f"round 0: mutual {history['rounds'][0]['mutual']} of {ref.MAX_RANK}, criterion "
                        f"{history['rounds'][0]['criterion']:.6f}")
    source.matrix.close(), target.matrix.close()

    # translate -a on the source as it is == translate on a source file aligned beforehand
    pq = g.ProductQuantizer.apply(case["target"].matrix, g.ProductQuantizerConfig(256, 8, 2))
    index = g.Index.sorted(case["target"].matrix, pq, "cosine")
    try:
        with open(paths["target.idx"], "wb") as fh:
            fh.write(dump_index(index, T_WORDS))
    finally:
        index.vector_index.close()
    write_vectors(paths["aligned.txt"], S_WORDS, learned.apply(case["x"]))

    def at_1(lines):
        return float(lines[0].split("@1 ")[1].split()[0])

    def translate(extra):
        out = io.BytesIO()
        assert cli.main(["translate", "-i", paths["target.idx"], "-e", paths["gold.txt"]] + extra, stdout=out) == 0
        return out.getvalue().decode("utf-8").splitlines()
    for method in (["--method", "nn"], ["--method", "csls"], ["--method", "csls", "-v", paths["target.txt"], "--exact"]):
        with_a = translate(method + ["-s", paths["source.txt"], "-a", paths["en-fr.map"]])
        before = translate(method + ["-s", paths["aligned.txt"]])
        unaligned = translate(method + ["-s", paths["source.txt"]])
        print(method, with_a, unaligned)
        assert with_a == before and len(with_a) == 1 and with_a[0].endswith(f"(n = {ref.N}, skipped 0)")
        # the map is what makes the source translatable: behind a rotation nobody told the target about, a source word
        # meets its translation by chance, one row in ref.N
        assert at_1(with_a) > at_1(unaligned) and at_1(unaligned) < 0.1
    with_a = translate(["-v", paths["target.txt"], "--exact", "-s", paths["source.txt"], "-a", paths["en-fr.map"]])
    w, _, _, _ = ref.train(case["x"], case["y"], case["seed_rows"], rounds=2)
    assert abs(at_1(with_a) - ref.precision_at_1(case["x"], case["y"], w, case["perm"])) <= 2 / ref.N + 5e-5   # 4 digits

    rotation.Rotation.identity(ref.D + 1).save(str(tmp_path / "other.map"))
    assert cli.main(["translate", "-i", paths["target.idx"], "-e", paths["gold.txt"], "-s", paths["source.txt"], "-a",
                     str(tmp_path / "other.map")], stdout=io.BytesIO()) == 1
    with open(paths["target.txt"], "w") as fh:                    # dimensions differ: reported, exit code 1
        fh.write("2 3\nt000 1 0 0\nt001 0 1 0\n")
    assert cli.main(["align", "-s", paths["source.txt"], "-t", paths["target.txt"], "--identical", "-o",
                     str(tmp_path / "never.map")], stdout=io.BytesIO()) == 1
    assert not (tmp_path / "never.map").exists()
