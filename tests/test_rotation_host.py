"""The host side of the rotated indexes (gulon_amd/rotation.py): the binding table, the eigenvalue allocation, Procrustes,
the file format, the numpy restatement of the kernel's arithmetic, and that the fixture of the device tests discriminates
(tests/rotation_ref.py).  No GPU."""
import functools
import itertools
import os
import re
import struct

import numpy as np
import pytest

import rotation_ref as ref
from gulon_amd import native, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gulon_dataset_rotate", "gulon_rotate_rows", "gulon_rotate_rows_dev", "gulon_dataset_moment"]


@functools.lru_cache(maxsize=None)
def trained(seed):
    """The restatement's training on the fixture: (data, queries, R float64, history)."""
    data, queries = ref.fixture(seed)
    R, history = ref.train_rotation(data)
    return data, queries, R, history


def random_orthogonal(d, seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(d, d)))
    return q * np.sign(np.diag(r))


def test_header_and_binding_table_carry_the_four_entry_points():
    header = open(os.path.join(ROOT, "include", "gulon_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint32_t %s\(" % name, header), name
    assert [len(native.SIGNATURES[n][1]) for n in NAMES] == [4, 6, 7, 3]
    L = native.lib()                                        # raises if the library lacks one of them
    assert all(hasattr(L, n) for n in NAMES)
    import gulon_amd
    for name in ("Rotation", "RotatedWordIndex", "train_rotation", "rotate_reference"):
        assert getattr(gulon_amd, name) is getattr(rotation, name) and name in gulon_amd.__all__


@pytest.mark.parametrize("d,m", [(10, 3), (8, 8), (32, 8), (7, 1)])
def test_eigenvalue_allocation_is_a_permutation_with_the_buckets_sizes(d, m):
    frm, until = ref.bounds(d, m)
    sizes = [u - f for f, u in zip(frm, until)]
    if (d, m) == (10, 3):
        assert sizes == [4, 3, 3]                           # ragged
    w = np.random.default_rng(d * 100 + m).lognormal(size=d)
    w[0] = 0.0                                              # clamped to the smallest positive double, not -inf
    w[-1] = -1e-9
    order = rotation.eigenvalue_allocation(w, sizes)
    assert sorted(order.tolist()) == list(range(d)) and order.dtype == np.int64
    assert order.tolist() == ref.allocation(w, sizes)
    # dealt largest first: within a bucket the eigenvalues descend, and bucket 0 holds the largest of all
    start = 0
    for s in sizes:
        bucket = w[order[start:start + s]]
        assert (np.diff(bucket) <= 0).all()
        start += s
    assert order[0] == int(np.argmax(w))
    with pytest.raises(ValueError):
        rotation.eigenvalue_allocation(w, [d + 1])


def test_eigenvalue_allocation_ties_go_to_the_lowest_bucket():
    # equal eigenvalues of log 0: every running sum stays 0, so each goes to the lowest bucket that is not full
    assert rotation.eigenvalue_allocation(np.ones(6), [2, 2, 2]).tolist() == [0, 1, 2, 3, 4, 5]
    # logs above 0: the three largest open the three buckets, the rest fill the emptiest from the back
    assert rotation.eigenvalue_allocation([64, 32, 16, 8, 4, 2], [2, 2, 2]).tolist() == [0, 5, 1, 4, 2, 3]


def test_greedy_allocation_is_within_its_bound_of_brute_force():
    """6 eigenvalues above 1 (logs l > 0) into 3 buckets of 2.  Let the greedy's heaviest bucket hold a, then b (b <= a:
    dealt later).  When b was dealt, that bucket had the smallest sum among the buckets not yet full, so a bucket that
    then held one item has it >= a and ends with >= a + l_min; a bucket that was full holds two items dealt before b,
    each >= b.  Either way the two other buckets end with >= b + l_min, so the mean bucket sum S / 3 is
    >= (a + b + 2 (b + l_min)) / 3, and no allocation's heaviest bucket is lighter than the mean:
    greedy_max - best_max <= a + b - S / 3 <= 2 (a - l_min) / 3 <= 2 (l_max - l_min) / 3."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        w = np.exp(rng.uniform(0.01, 6.0, 6))
        logs = np.log(w)
        order = rotation.eigenvalue_allocation(w, [2, 2, 2])
        greedy = max(logs[order[i:i + 2]].sum() for i in (0, 2, 4))
        best = min(max(logs[list(p[i:i + 2])].sum() for i in (0, 2, 4)) for p in itertools.permutations(range(6)))
        assert best - 1e-12 <= greedy <= best + 2.0 * (logs.max() - logs.min()) / 3.0 + 1e-12


def test_procrustes_returns_an_orthogonal_matrix_unchanged():
    for d, seed in ((1, 0), (5, 1), (32, 2)):
        A = random_orthogonal(d, seed)
        assert np.abs(rotation.procrustes(A) - A).max() <= 1e-12
    # and solves the problem it is named for: Y = X A recovers A
    X = np.random.default_rng(3).normal(size=(100, 6))
    A = random_orthogonal(6, 4)
    assert np.abs(rotation.procrustes(X.T @ (X @ A)) - A).max() <= 1e-12


def test_a_trained_float32_rotation_is_orthogonal_to_rounding():
    """Casting a float64-orthogonal matrix moves each entry by <= 2^-25 relative; Cauchy-Schwarz on a pair of columns
    gives <= 2^-23 ... the bound of the issue: 2^-22 with a factor of two for the SVD."""
    for seed in (1, 2, 3):
        R = trained(seed)[2]
        rot = rotation.Rotation(R)
        assert rot.matrix.dtype == np.float32 and rot.dimension == ref.D
        assert rot.orthogonality_error() <= 2.0 ** -22
    assert rotation.Rotation.identity(7).orthogonality_error() == 0.0
    assert rotation.Rotation(2 * np.eye(3)).orthogonality_error() == 3.0
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((0, 0))):
        with pytest.raises(ValueError):
            rotation.Rotation(bad)


def test_file_round_trip_and_malformed_files(tmp_path):
    R = np.random.default_rng(0).normal(size=(5, 5)).astype(np.float32)
    R[0, 0], R[1, 1] = -0.0, np.float32(1e-42)             # a negative zero and a subnormal keep their bits
    path = tmp_path / "r.rot"
    rotation.Rotation(R).save(path)
    raw = path.read_bytes()
    assert raw[:8] == b"GULONROT" and struct.unpack("<II", raw[8:16]) == (1, 5) and len(raw) == 16 + 100
    assert raw[16:] == R.astype("<f4").tobytes()
    back = rotation.Rotation.load(path)
    assert np.array_equal(back.matrix.view(np.uint32), R.view(np.uint32))

    def rejected(data, match):
        bad = tmp_path / "bad.rot"
        bad.write_bytes(data)
        with pytest.raises(ValueError, match=match):
            rotation.Rotation.load(bad)
    rejected(b"GULONROX" + raw[8:], "not a rotation file")
    rejected(raw[:8] + struct.pack("<I", 2) + raw[12:], "version 2")
    rejected(raw[:-1], "bytes of matrix")
    rejected(raw[:16], "bytes of matrix")
    rejected(raw[:7], "not a rotation file")
    rejected(b"", "not a rotation file")
    rejected(raw + b"\0", "bytes of matrix")
    rejected(raw[:8] + struct.pack("<II", 1, 0), "bytes of matrix")
    for value in (np.nan, np.inf, -np.inf):
        broken = R.copy()
        broken[3, 2] = value
        rejected(raw[:16] + broken.tobytes(), "non-finite")


def test_rotate_reference_is_the_stated_arithmetic():
    rng = np.random.default_rng(1)
    x, R = rng.normal(size=(3, 4)).astype(np.float32), rng.normal(size=(4, 4)).astype(np.float32)
    for transpose in (False, True):
        got = rotation.rotate_reference(x, R, transpose)
        for i in range(3):
            for c in range(4):
                s = np.float32(0)
                for j in range(4):
                    s = np.float32(s + np.float32(x[i, j] * (R[c, j] if transpose else R[j, c])))
                assert got[i, c].view(np.uint32) == s.view(np.uint32)
    assert rotation.rotate_reference(x[0], R).shape == (4,)
    assert rotation.rotate_reference(np.zeros((0, 4), np.float32), R).shape == (0, 4)


@pytest.mark.parametrize("d", [1, 5, 32, 300])
def test_rotating_there_and_back_returns_the_vector(d):
    R = random_orthogonal(d, d).astype(np.float32)
    x = (np.random.default_rng(d).normal(size=(17, d)) * 3).astype(np.float32)
    back = rotation.rotate_reference(rotation.rotate_reference(x, R), R, transpose=True)
    assert np.abs(back.astype(np.float64) - x).max() <= 4 * d * 2.0 ** -24 * np.abs(x).max()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_fixture_discriminates(seed):
    """The restatement on the fixture: the rotation cuts the quantization error to a quarter or less and lifts recall@10
    by 0.3 or more (measured: 0.147-0.161 of the error, +0.41-0.43 of recall)."""
    data, queries, R, history = trained(seed)
    ratio = min(history["rounds"]) / history["identity"]
    plain = ref.recall_at(data, queries, np.eye(ref.D))
    rotated = ref.recall_at(data, queries, R)
    print(f"seed {seed}: E_rotated / E_identity = {ratio:.4f}, recall@10 plain {plain:.4f}, rotated {rotated:.4f}")
    assert history["chosen"] != "identity"
    assert ratio <= 0.25
    assert rotated >= plain + 0.3
    assert all(b < a for a, b in zip(history["rounds"], history["rounds"][1:3]))    # the first rounds refine
