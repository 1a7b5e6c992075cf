"""The fixture of the alignment tests and a float64 numpy restatement of gulon_amd.alignment's pipeline -- seed solve,
CSLS dictionary induction restricted to the first max_rank rows of either side, mutual pairs, Procrustes against the
original source rows, the criterion and the choice -- for tests/test_gpu_alignment.py.  Nothing here touches the device."""
import numpy as np

N, D, CENTRES, SPREAD, NOISE = 512, 32, 32, 0.35, 0.05
SEED_PAIRS, SEED_WRONG = 40, 10
ROUNDS, MAX_RANK, NEIGHBOURS = 3, 384, 10
CRITERION_ROWS = 10000


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def fixture(seed):
    """-> (X [N][D] float32, Y [N][D] float32, perm, Q, seed pairs [(source row, target row)]).  Y: unit rows around
    CENTRES unit centres (spread SPREAD per coordinate); X = unit(Y[perm] Q^T + NOISE * noise), noise standard normal
    per coordinate, for an orthogonal Q, so that X Q ~ Y[perm]: source row i translates to target row perm[i].  The seed pairs:
    SEED_PAIRS source rows among the first MAX_RANK, SEED_WRONG of them paired with a target row that is not theirs."""
    rng = np.random.default_rng([seed, N, D])
    centres = unit(rng.normal(size=(CENTRES, D)))
    y = unit(centres[rng.integers(0, CENTRES, N)] + SPREAD * rng.normal(size=(N, D)))
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    perm = rng.permutation(N)
    x = unit(y[perm] @ q.T + NOISE * rng.normal(size=(N, D)))
    rows = rng.choice(MAX_RANK, SEED_PAIRS, replace=False)
    pairs = [(int(s), int(perm[s])) for s in rows]
    for j in range(SEED_WRONG):
        s, t = pairs[j]
        pairs[j] = (s, int((t + 1 + rng.integers(0, N - 1)) % N))                  # any row but the right one
    return x.astype(np.float32), y.astype(np.float32), perm, q, pairs


def procrustes(moment):
    u, _, vt = np.linalg.svd(moment)
    return u @ vt


def seed_map(x, y, pairs):
    s, t = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return procrustes(x[s].astype(np.float64).T @ y[t].astype(np.float64))


def induce(x, y, w, max_rank, neighbours):
    """-> (fwd [Rs], match [Rs]): every source row's CSLS best target row among the first max_rank of either side, and
    the same where the target row's best source row is that source row, else -1."""
    s, t = unit((x @ w)[:max_rank]), unit(y[:max_rank])
    cos = s @ t.T
    k_t, k_s = min(neighbours, len(s)), min(neighbours, len(t))
    r_t = np.sort(cos, axis=0)[-k_t:].mean(axis=0)                # per target row: its nearest source rows
    r_s = np.sort(cos, axis=1)[:, -k_s:].mean(axis=1)
    fwd = np.argmax(2 * cos - r_t[None, :], axis=1)               # the query's own r shifts all its scores alike
    bwd = np.argmax(2 * cos - r_s[:, None], axis=0)
    match = np.where(bwd[fwd] == np.arange(len(s)), fwd, -1)
    return fwd, match


def train(x, y, pairs, rounds=ROUNDS, max_rank=MAX_RANK, neighbours=NEIGHBOURS):
    """-> (the chosen map, its round, [(mutual, criterion) per round], every round's map)."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    w = seed_map(x, y, pairs)
    maps, history = [], []
    for t in range(rounds + 1):
        fwd, match = induce(x64, y64, w, max_rank, neighbours)
        v = min(len(fwd), CRITERION_ROWS)
        criterion = float(np.einsum("ij,ij->i", x64[:v] @ w, y64[fwd[:v]]).mean())
        live = np.flatnonzero(match >= 0)
        maps.append(w)
        history.append((len(live), criterion))
        if t == rounds or not len(live):
            break
        w = procrustes(x64[live].T @ y64[match[live]])
    chosen = int(np.argmax([c for _, c in history]))
    return maps[chosen], chosen, history, maps


def precision_at_1(x, y, w, perm):
    """Plain nearest neighbours of every mapped source row among ALL target rows: the share that is the row's own."""
    cos = unit(x.astype(np.float64) @ w) @ unit(y.astype(np.float64)).T
    return float((np.argmax(cos, axis=1) == perm).mean())
