"""The fixture of the rotation tests and a numpy float64 restatement of gulon_amd.rotation.train_rotation with a Lloyd
k-means of its own.  No GPU, no gulon_amd: the device tests compare against this, the host tests check that the fixture
discriminates (a rotation must matter on it)."""
import numpy as np

N, D, M, K, ITERATIONS, QUERIES = 2048, 32, 8, 16, 10, 200


def fixture(seed, n=N, d=D):
    """(data [n][d], queries [200][d]) float32: 64 Gaussian clusters, coordinate e scaled by 0.85 ** e."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(64, d))
    rows = cen[rng.integers(0, 64, n + QUERIES)] + 0.5 * rng.normal(size=(n + QUERIES, d))
    rows = (rows * 0.85 ** np.arange(d)).astype(np.float32)
    return rows[:n], rows[n:]


def bounds(d, m):
    """Vectors.subvectors: the first d - m * (ceil(d / m) - 1) runs have ceil(d / m) coordinates, the rest one fewer."""
    ideal = -(-d // m)
    full = m - (ideal * m - d)
    sizes = [ideal if i < full else ideal - 1 for i in range(m)]
    until = np.cumsum(sizes)
    return (until - sizes).tolist(), until.tolist()


def lloyd(x, k, iterations, rng):
    """Lloyd's k-means from k distinct rows; an empty cluster keeps its centroid.  -> centroids [k][s] float64."""
    cents = x[rng.choice(len(x), size=min(k, len(x)), replace=False)].copy()
    for _ in range(iterations):
        assign = ((x[:, None, :] - cents[None, :, :]) ** 2).sum(-1).argmin(1)
        for c in range(len(cents)):
            members = x[assign == c]
            if len(members):
                cents[c] = members.mean(0)
    return cents


def quantize(x, m=M, k=K, iterations=ITERATIONS, seed=0):
    """Train a product quantizer on x (float64) and encode x with it.  -> (code books, codes [n][m], decoded [n][d])."""
    rng = np.random.default_rng(seed)
    frm, until = bounds(x.shape[1], m)
    books, codes, decoded = [], np.zeros((len(x), m), np.int64), np.zeros_like(x)
    for j, (f, u) in enumerate(zip(frm, until)):
        cents = lloyd(x[:, f:u], k, iterations, rng)
        codes[:, j] = ((x[:, None, f:u] - cents[None, :, :]) ** 2).sum(-1).argmin(1)
        decoded[:, f:u] = cents[codes[:, j]]
        books.append(cents)
    return books, codes, decoded


def allocation(eigenvalues, sizes):
    """The greedy deal of eigenvalue_allocation, restated."""
    w = np.asarray(eigenvalues, np.float64)
    logs = np.log(np.maximum(w, np.nextafter(0.0, 1.0)))
    buckets, sums = [[] for _ in sizes], np.zeros(len(sizes))
    for i in np.argsort(-w, kind="stable"):
        open_ = [b for b in range(len(sizes)) if len(buckets[b]) < sizes[b]]
        b = min(open_, key=lambda b: (sums[b], b))
        buckets[b].append(int(i))
        sums[b] += logs[i]
    return [i for bucket in buckets for i in bucket]


def procrustes(moment):
    u, _, vt = np.linalg.svd(moment)
    return u @ vt


def train_rotation(x, m=M, k=K, iterations=ITERATIONS, rounds=4, seed=0):
    """-> (R float64, {"identity": E_id, "rounds": [E_0 ...], "chosen": t or "identity"}), errors as float64 sums."""
    x = np.asarray(x, np.float64)
    frm, until = bounds(x.shape[1], m)
    w, v = np.linalg.eigh(x.T @ x)
    R = v[:, allocation(w, [u - f for f, u in zip(frm, until)])]
    candidates, errors = [], []
    for t in range(rounds + 1):
        xr = x @ R
        _, _, y = quantize(xr, m, k, iterations, seed)
        candidates.append(R)
        errors.append(float(((xr - y) ** 2).sum()))
        if t != rounds:
            R = procrustes(x.T @ y)
    _, _, y = quantize(x, m, k, iterations, seed)
    identity = float(((x - y) ** 2).sum())
    best = int(np.argmin(errors))
    if not errors[best] < identity:
        return np.eye(x.shape[1]), {"identity": identity, "rounds": errors, "chosen": "identity"}
    return candidates[best], {"identity": identity, "rounds": errors, "chosen": best}


def exact_neighbours(data, queries, k):
    d2 = ((np.asarray(queries, np.float64)[:, None, :] - np.asarray(data, np.float64)[None, :, :]) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def recall(found, truth):
    """The mean share of truth's rows that `found` holds, row by row."""
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / len(t) for f, t in zip(found, truth)]))


def recall_at(data, queries, R, k_nn=10, m=M, k=K, iterations=ITERATIONS, seed=0):
    """recall@k_nn of a quantizer trained on data @ R, queried with queries @ R, against the exact neighbours of the
    original vectors."""
    x, q = np.asarray(data, np.float64) @ R, np.asarray(queries, np.float64) @ R
    _, _, y = quantize(x, m, k, iterations, seed)
    return recall(exact_neighbours(y, q, k_nn), exact_neighbours(data, queries, k_nn))


def procrustes_gain(x, decoded):
    """What one Procrustes step gains with the codes held fixed: sum |x - y|^2 - sum |x R' - y|^2, R' = procrustes(x^T y),
    in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(decoded, np.float64)
    R = procrustes(x.T @ y)
    return float(((x - y) ** 2).sum() - ((x @ R - y) ** 2).sum())
