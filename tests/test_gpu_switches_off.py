"""The process-wide switches of the native library: the ones that turn a fast path off so that a
wrong result can be bisected to it, GULON_KMEANS_SERIAL, GULON_HOST_CONTEXTS, and the synchronous statistics.  A
fallback nobody runs rots, and then bisecting lies.

Each switch is read once per process, so each gets ONE fresh child (tests/switch_children.py), started as
test_pq_train_with_stream_update_off starts its own, one after the other, with the switch -- and the ScanTuning keys
its handles are to read at creation -- in its environment.  The child writes raw answers to an .npz; this process
computes the oracle's and compares."""
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_ref as mr
import switch_children as sc
from conftest import bits
from test_gpu_query import _same_up_to_ties
from test_gpu_scan_thresholds import _nearest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import switch_children; switch_children.main(sys.argv[3:])"
SMALL_FILTER = {"GULON_FILTER_MIN_RB": "4", "GULON_FILTER_PERIOD": "8", "GULON_FILTER_STAGE0": "1",
                "GULON_FILTER_STAGE1": "2", "GULON_FILTER_SAMPLE": "512"}       # test_gpu_filter's `tune`

pytestmark = pytest.mark.gpu


def run_child(tmp_path, what, inputs, env, timeout):
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **inputs)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, TESTS, what, src, dst],
                       env={**os.environ, **env}, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    with np.load(dst) as z:
        return {key: z[key] for key in z.files}, r.stderr


def raw(out, label):
    return tuple(out[f"{label}/{name}"] for name in ("i", "d", "c", "f"))


def all_distances(oracle, cents, idx, d, k, Q):
    """Every row's distance from the oracle's tables, summed quantizer by quantizer in binary32.  [B][n]."""
    m, n = idx.shape
    T = oracle.prepare_query(cents, d, m, k, Q)
    out = np.zeros((len(Q), n), np.float32)
    for q in range(len(Q)):
        acc = np.zeros(n, np.float32)
        for j in range(m):
            acc = acc + T[q, j][idx[j]]
        out[q] = acc
    return out


def check_flat(got, oi, od, oc, replayed_only=False):
    """test_gpu_query._check on raw outputs: distance bits and counts; rows where no tie was flagged or the flagged tie
    was replayed, else the same rows up to the ties."""
    gi, gd, gc, gf = got
    assert np.array_equal(gc, oc)
    for q in range(len(oc)):
        c = oc[q]
        assert np.array_equal(bits(gd[q, :c]), bits(od[q, :c])), q
        if gf[q] == 0 or (gf[q] & 4):
            assert gi[q, :c].tolist() == oi[q, :c].tolist(), q
        else:
            assert not replayed_only, (q, gf[q])
            _same_up_to_ties(gi[q, :c], gd[q, :c], oi[q, :c])


def same_answers(a, b, what):
    ai, ad, ac, af = a
    bi, bd, bc, bf = b
    assert np.array_equal(ac, bc) and np.array_equal(af, bf), what
    for q in range(len(ac)):
        assert np.array_equal(ai[q, :ac[q]], bi[q, :ac[q]]) and np.array_equal(bits(ad[q, :ac[q]]), bits(bd[q, :ac[q]])), (what, q)


# ---- GULON_FILTER_ORDER_WINDOW=0: the only way into the exact scan's walk over the conflict-ordered copy ------------------

def test_order_window_off(oracle, tmp_path):
    """The ordered copy orders single 64-row blocks; launch_scan_p then hands it, with the lanes' places, to the exact
    scan: plain, peeled and partial-list scans map a lane to its row through the places and test the range on that row.
    Ranges cut the first and the last block or lie inside one block; B = 17 is three tiles.  Everything equals the oracle
    and the same handle on the plain copy (GULON_FILTER_ORDER=0).  (64, 32, 256) is never ordered: the control."""
    n, B = 70000, 17
    worlds = {"plainidx": (128, 16, 256, 0), "dupidx": (128, 16, 256, 30000), "control": (64, 32, 256, 0)}
    inputs, data = {}, {}
    for name, (d, m, k, dup) in worlds.items():
        cents, idx = sc.random_index(n, d, m, k, seed=len(name) + d, dup=dup)
        Q = np.random.default_rng(5).standard_normal((B, d)).astype(np.float32)
        if dup:      # decoded rows with a twin: two rows at distance 0
            for q in range(0, B, 2):
                Q[q] = sc.decode(cents, k, idx[:, 100 + q], oracle.subvectors(d, m))
        inputs.update({name + "_cents": cents, name + "_idx": idx, name + "_Q": Q, name + "_dk": np.array([d, k])})
        data[name] = (cents, idx, Q, d, k)
    out, _ = run_child(tmp_path, "order_window", inputs, {**SMALL_FILTER, "GULON_FILTER_ORDER_WINDOW": "0"}, 300)
    ranges = {label: (frm, until) for label, frm, until in sc.order_window_ranges(n)}
    for name, (cents, idx, Q, d, k) in data.items():
        dist = all_distances(oracle, cents, idx, d, k, Q)
        cuts = [label for label, frm, until in sc.order_window_ranges(n)]
        labels = [f"filtered/{r}" for r in cuts[:2]]                                                       # (a)
        labels += [f"exact/{blocks}/{K}/{r}" for blocks in (1, 4096) for K in (1, 10, 63) for r in cuts]    # (b)
        labels += [f"peeled/{K}/{r}" for K in (100, 200) for r in cuts[:2]]                                # (c)
        labels += ["partial/low", "partial/high"]                                                          # (d)
        for label in labels:
            parts = label.split("/")
            o, p = f"{name}/ordered/{label}", f"{name}/plain/{label}"
            if parts[0] == "partial":
                frm, until = (0, sc.ORDER_WINDOW_SPLIT) if parts[1] == "low" else (sc.ORDER_WINDOW_SPLIT, n)
                for q in range(B):
                    dd, rows = _nearest(dist[q], frm, until, 11)
                    e = mr.order(dd, rows)[:11]
                    assert np.array_equal(out[o + "/i"][q], rows[e]) and np.array_equal(bits(out[o + "/v"][q]), bits(dd[e])), (label, q)
                assert np.array_equal(out[o + "/i"], out[p + "/i"]) and np.array_equal(bits(out[o + "/v"]), bits(out[p + "/v"]))
                continue
            K = 10 if parts[0] == "filtered" else int(parts[-2])
            frm, until = ranges[parts[-1]]
            got = raw(out, o)
            oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K, frm, until)
            if K <= 63:
                check_flat(got, oi, od, oc)
            else:
                for q in range(B):
                    ei, ed, ec, ef = mr.peel_final(*mr.peeled_rounds(*_nearest(dist[q], frm, until, K + 65), K), K)
                    assert got[2][q] == ec == oc[q] and got[3][q] == ef, (label, q)
                    assert np.array_equal(got[0][q, :ec], ei[:ec]) and np.array_equal(bits(got[1][q, :ec]), bits(ed[:ec])), (label, q)
                    assert np.array_equal(bits(ed[:ec]), bits(od[q, :ec]))
            same_answers(got, raw(out, p), label)
        for mode in ("ordered", "plain"):
            assert out[f"{name}/{mode}/filtered/whole/tiles"] > 0 and out[f"{name}/{mode}/filtered/cut/tiles"] > 0
            assert out[f"{name}/{mode}/exact_tiles"] == 0


# ---- GULON_TIE_REPLAY=0 -------------------------------------------------------------------------------------------------

def flat_cases(oracle, cases):
    """cases: (cents, idx, Q, d, k, K, from, until, repeats) -> the child's inputs."""
    inputs = {"cases": np.array(len(cases))}
    for c, (cents, idx, Q, d, k, K, frm, until, reps) in enumerate(cases):
        inputs.update({f"c{c}_cents": cents, f"c{c}_idx": idx, f"c{c}_Q": Q,
                       f"c{c}_params": np.array([d, k, K, frm, until, reps])})
    return inputs


def test_tie_replay_off(oracle, tmp_path):
    """No replay of flagged queries: distances and counts are still the oracle's, no answer says it was replayed (flag 4),
    a flagged answer holds the oracle's rows up to its ties, an unflagged one exactly."""
    cases = []
    for n, d, m, k, K, dup in [(6000, 16, 4, 16, 9, 3000), (40000, 32, 8, 4, 10, 0), (20000, 64, 16, 256, 10, 0),
                               (70000, 128, 16, 256, 10, 30000)]:
        cents, idx = sc.random_index(n, d, m, k, seed=n + K, dup=dup)
        Q = np.random.default_rng(K).standard_normal((7, d)).astype(np.float32)
        cases.append((cents, idx, Q, d, k, K, 0, n, 1))
    out, _ = run_child(tmp_path, "flat", flat_cases(oracle, cases), {"GULON_TIE_REPLAY": "0"}, 180)
    flagged = []
    for c, (cents, idx, Q, d, k, K, frm, until, reps) in enumerate(cases):
        got = raw(out, f"c{c}/r0")
        assert not (got[3] & 4).any()
        check_flat(got, *oracle.pq_batch_query(idx, d, k, cents, Q, K, frm, until))
        flagged.append(int((got[3] != 0).sum()))
    assert flagged[0] == 7 and flagged[1] == 7 and flagged[2] == 0 and flagged[3] > 0, flagged     # tie-heavy, tie-free


# ---- GULON_REPLAY_L1_FILTER=0 -------------------------------------------------------------------------------------------

def test_replay_l1_filter_off(oracle, tmp_path):
    """The tie replay's first level by the segment scan where the filter would have taken it: rows equal the reference
    heap's, and every flagged tie was replayed."""
    cases = []
    for n, d, m, k, K, dup, frm, until in [(6000, 16, 4, 16, 9, 3000, 0, None), (40000, 32, 8, 4, 10, 0, 0, None),
                                           (30000, 16, 16, 2, 63, 0, 5, 29990), (2000, 8, 2, 3, 5, 0, 0, None)]:
        cents, idx = sc.random_index(n, d, m, k, seed=n + K, dup=dup)
        Q = np.random.default_rng(K).standard_normal((5, d)).astype(np.float32)
        cases.append((cents, idx, Q, d, k, K, frm, n if until is None else until, 1))
    n, d, m, k, K, B, nbase, frm, until = 260000, 64, 16, 256, 5, 70, 300, 1000, 255000      # many flagged, long range
    cents, idx, Q = sc.many_flagged_index(n, d, m, k, K, B, nbase, oracle.subvectors(d, m))
    cases.append((cents, idx, Q, d, k, K, frm, until, 2))       # twice: the second batch knows that many were flagged
    out, _ = run_child(tmp_path, "flat", flat_cases(oracle, cases), {"GULON_REPLAY_L1_FILTER": "0"}, 240)
    for c, (cents, idx, Q, d, k, K, frm, until, reps) in enumerate(cases):
        oi, od, oc = oracle.pq_batch_query(idx, d, k, cents, Q, K, frm, until)
        for r in range(reps):
            got = raw(out, f"c{c}/r{r}")
            tied = (got[3] & 3) != 0
            assert ((got[3] & 4) != 0)[tied].all()
            check_flat(got, oi, od, oc, replayed_only=True)
            if reps == 2:
                assert tied.sum() >= 32


# ---- GULON_GROUPED_FILTER=0 ---------------------------------------------------------------------------------------------

def check_grouped(oracle, out, label, d, k, Q, K, limit):
    ei, ed, ec = oracle.grouped_query(out[label + "/codes"], d, k, out[label + "/pq"], out[label + "/gcents"],
                                      out[label + "/offsets"], Q, K, 0, limit)
    oi, od, oc = out[label + "/i"], out[label + "/d"], out[label + "/c"]
    assert np.array_equal(oc, ec)
    for q in range(len(Q)):
        assert oi[q, :oc[q]].tolist() == ei[q, :ec[q]].tolist(), (label, q)
        assert np.array_equal(bits(od[q, :oc[q]]), bits(ed[q, :ec[q]])), (label, q)


def grouped_case(n, d, groups, m, k, limit, dup, B, K, iters=2):
    X = sc.grouped_data(n, d, n + groups, dup)
    rng = np.random.default_rng(5)
    Q = np.concatenate([X[rng.integers(0, n, B - 2)], (rng.standard_normal((2, d)) * 3).astype(np.float32)])
    return X, Q, np.array([groups, m, k, iters, limit, K])


def test_grouped_filter_off(oracle, tmp_path):
    """Two shapes of test_by_group_filter_equals_reference, one with duplicated rows, without the by-group 8-bit filter:
    the oracle's grouped query, on the codes, codebooks and groups the child built."""
    shapes = [(60000, 24, 300, 8, 64, 90, 3000), (66000, 8, 3000, 4, 16, 100, 0)]
    inputs, keep = {"cases": np.array(len(shapes))}, []
    for c, (n, d, groups, m, k, limit, dup) in enumerate(shapes):
        X, Q, params = grouped_case(n, d, groups, m, k, limit, dup, 40, 10)
        inputs.update({f"c{c}_X": X, f"c{c}_Q": Q, f"c{c}_params": params})
        keep.append((d, k, Q, 10, limit))
    out, err = run_child(tmp_path, "grouped", inputs, {"GULON_GROUPED_FILTER": "0", "GULON_GROUPED_STATS": "1"}, 240)
    assert "by-group filter" not in err and "approximate pre-selection" in err
    for c, (d, k, Q, K, limit) in enumerate(keep):
        check_grouped(oracle, out, f"c{c}", d, k, Q, K, limit)


# ---- GULON_KMEANS_NO_MFMA=1, GULON_KMEANS_SERIAL=1 ----------------------------------------------------------------------

def kmeans_cases():
    from test_gpu_kmeans import _clustered
    dup = _clustered(11, 6000, 24)
    dup[3000:] = dup[:3000]                      # duplicated rows: equal distances, the tie-break stream is drawn
    return [(_clustered(20000, 20000, 32), 4, 256, 2),
            (_clustered(9000, 9000, 64), 1, 33, 2),          # the streaming assign's shape: s = 64, k = 33
            (dup, 1, 40, 2)]


def check_kmeans(oracle, out, label, X, m, k, iters):
    cents, _, _ = oracle.pq_train(X, m, k, iters)
    assert np.array_equal(bits(out[label + "/cents"]), bits(cents)), label
    assert np.array_equal(out[label + "/codes"], oracle.pq_encode(X, m, k, cents)), label


@pytest.mark.parametrize("switch", ["GULON_KMEANS_NO_MFMA", "GULON_KMEANS_SERIAL"])
def test_kmeans_switches(oracle, tmp_path, switch):
    """ProductQuantizer.apply and encode bit for bit without the matrix cores / with every sub-quantizer on one stream."""
    cases = kmeans_cases()
    inputs = {"cases": np.array(len(cases))}
    for c, (X, m, k, iters) in enumerate(cases):
        inputs.update({f"c{c}_X": X, f"c{c}_params": np.array([m, k, iters])})
    out, _ = run_child(tmp_path, "kmeans", inputs, {switch: "1"}, 240)
    for c, (X, m, k, iters) in enumerate(cases):
        check_kmeans(oracle, out, f"c{c}", X, m, k, iters)


# ---- GULON_HOST_CONTEXTS -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("contexts", [1, 3])
def test_host_contexts(oracle, tmp_path, contexts):
    """Eight threads on one handle with one workspace (they take turns) and with three."""
    n, d, m, k, K = 70000, 32, 8, 256, 10
    cents, idx = sc.random_index(n, d, m, k, seed=4)
    rng = np.random.default_rng(2)
    Qs = [rng.standard_normal((7 + t, d)).astype(np.float32) for t in range(8)]
    inputs = {"cents": cents, "idx": idx, "params": np.array([d, k, K]), **{f"Q{t}": Qs[t] for t in range(8)}}
    out, _ = run_child(tmp_path, "host_contexts", inputs, {"GULON_HOST_CONTEXTS": str(contexts)}, 180)
    for t in range(8):
        check_flat(raw(out, f"t{t}"), *oracle.pq_batch_query(idx, d, k, cents, Qs[t], K))


# ---- the synchronous statistics, all at once -------------------------------------------------------------------------------

def test_statistics_switches_change_no_answer(oracle, tmp_path):
    """GULON_FILTER_STATS, GULON_REPLAY_STATS, GULON_GROUPED_STATS and GULON_TRACE together: a filtered query, a tie query,
    a grouped query and a small k-means answer as ever, and something is printed."""
    inputs, K = {}, 10
    flat = {"filtered": (60000, 128, 16, 256, 0), "ties": (6000, 16, 4, 16, 3000)}
    keep = {}
    for name, (n, d, m, k, dup) in flat.items():
        cents, idx = sc.random_index(n, d, m, k, seed=n, dup=dup)
        Q = np.random.default_rng(1).standard_normal((9, d)).astype(np.float32)
        inputs.update({name + "_cents": cents, name + "_idx": idx, name + "_Q": Q, name + "_params": np.array([d, k, K])})
        keep[name] = (cents, idx, Q, d, k)
    gd, gk, glimit = 16, 16, 5
    X, GQ, params = grouped_case(6000, gd, 12, 4, gk, glimit, 0, 9, 5, iters=3)
    inputs.update({"grouped_X": X, "grouped_Q": GQ, "grouped_params": params})
    from test_gpu_kmeans import _clustered
    KX = _clustered(3, 3000, 16)
    inputs.update({"kmeans_X": KX, "kmeans_params": np.array([2, 16, 2])})
    env = {**SMALL_FILTER, "GULON_FILTER_STATS": "1", "GULON_REPLAY_STATS": "1", "GULON_GROUPED_STATS": "1",
           "GULON_TRACE": "1"}
    out, err = run_child(tmp_path, "stats", inputs, env, 240)
    assert err.strip()
    for name, (cents, idx, Q, d, k) in keep.items():
        got = raw(out, name)
        check_flat(got, *oracle.pq_batch_query(idx, d, k, cents, Q, K))
    assert out["filtered/tiles"] > 0
    assert ((raw(out, "ties")[3] & 4) != 0).all()
    check_grouped(oracle, out, "grouped", gd, gk, GQ, 5, glimit)
    check_kmeans(oracle, out, "kmeans", KX, 2, 16, 2)
