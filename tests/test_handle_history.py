"""The sequences of handle_history.py are neither vacuous nor lenient -- checked on the CPU, against the oracle alone,
for every form and every sequence test_gpu_handle_history.py plays.  Where a seed misses a condition the seed or the
generator changes, never the condition."""
import numpy as np
import pytest

import handle_history as hh
import replay_adversary as ra
import value_regimes as vr


def _batches(w, kinds=("query",)):
    """the distinct calls of the four sequences of a world"""
    seen = {}
    for seq in hh.sequences(w).values():
        for _, call in seq:
            if call.kind in kinds:
                seen[call] = True
    return list(seen)


def _inside(w, call):
    return 0 <= call.frm < call.until <= w.n and call.B > 0 and call.K > 0


def _top(oracle, w, call, depth):
    """[B][c] the `depth` smallest distances of every query of the call over its range, ascending"""
    Q = hh.queries(oracle, w, call)
    with np.errstate(invalid="ignore"):
        oi, od, oc = oracle.pq_batch_query(w.idx, w.d, w.k, w.cents, Q, depth, call.frm, call.until)
    assert (oc == min(depth, call.until - call.frm)).all()
    return np.sort(od[:, :oc[0]], axis=1)


def _tied(top):
    return np.array([(v[1:] == v[:-1]).any() for v in top])


def test_forms_are_the_value_regime_shapes():
    assert hh.FORMS == {name: vr.FORMS[name] for name in ("m16", "m25", "m64", "k5", "w1024", "w5000")}
    assert hh.BYTE_FORMS == ("m16", "m25", "m64", "k5")
    for name in hh.FORMS:
        w = hh.world(name)
        assert len(w.pairs) == ra.PAIRS
        for a, b in w.pairs:
            assert a != b and np.array_equal(w.idx[:, a], w.idx[:, b])
        # under TUNE the whole index and the probes' sub-range take the filter: at least FILTER_MIN_RB and one PERIOD of
        # row blocks (eight times that for 16-bit codes)
        lo, hi = vr.sub_range(w.n)
        need = max(hh.TUNE["GULON_FILTER_MIN_RB"], hh.TUNE["GULON_FILTER_PERIOD"]) * (8 if w.k > 256 else 1)
        assert (hi + 63) // 64 - lo // 64 >= need


@pytest.mark.parametrize("name", [f for f in hh.FORMS if f != "k5"])
def test_gauss_batches_have_no_ties(oracle, name):
    """no two equal distances among the K + 1 smallest (K + 2 for a partial list): ids are compared exactly for every
    query of these batches, wide and peeled calls included"""
    w = hh.world(name)
    calls = [c for c in _batches(w, ("query", "partial", "bounded")) if c.qkind == "gauss" and _inside(w, c)]
    assert len(calls) >= 10 and any(c.K > hh.MAX_K for c in calls)
    for call in calls:
        top = _top(oracle, w, call, hh.depth_of(call) + 1)
        assert not _tied(top).any(), call
        if call.kind == "query":
            assert not hh.expected(oracle, w, call).tie.any(), call


@pytest.mark.parametrize("name", list(hh.FORMS))
def test_tied_batches_tie(oracle, name):
    w = hh.world(name)
    calls = [c for c in _batches(w) if c.qkind == "tied" and _inside(w, c)]
    assert any(c.B == 40 for c in calls)
    for call in calls:
        tied = _tied(_top(oracle, w, call, call.K + 1))
        assert hh.expected(oracle, w, call).tie.tolist() == tied.tolist()
        if call.B == 40:
            assert tied.sum() >= 32, (call, int(tied.sum()))
        if call.B == 1 and call.K >= 2:
            assert tied.all(), call


def test_k5_gauss_batches_all_tie(oracle):
    """625 distinct codes in 20 000 rows: every query ties, its batches are compared as the tied ones are"""
    w = hh.world("k5")
    calls = [c for c in _batches(w) if c.qkind == "gauss" and _inside(w, c) and c.until - c.frm > 5000]
    assert len(calls) >= 10
    for call in calls:
        assert _tied(_top(oracle, w, call, call.K + 1)).all(), call


@pytest.mark.parametrize("name", hh.BYTE_FORMS)
def test_byte_form_batches_stay_inside_the_replay_limits(oracle, name):
    """every tied query of a byte form at K <= 63 makes at most KEEP insertions and has at most POOL candidates: the
    GPU test then demands the exact replay of every flagged query, and compares its ids exactly"""
    w = hh.world(name)
    checked = 0
    for call in _batches(w, ("query", "query_rows")):
        if not _inside(w, call) or call.K > hh.MAX_K:
            continue
        want = hh.expected(oracle, w, call)
        Q = hh.queries(oracle, w, call)
        for q in np.flatnonzero(want.tie):
            if not np.isfinite(want.od[q, :want.oc[q]]).all():
                continue
            ins, cand = hh.replay_load(oracle, w, Q[q], call.K, call.frm, call.until)
            assert ins <= ra.KEEP and cand <= ra.POOL, (call, int(q), ins, cand)
            checked += 1
    assert checked >= 40


@pytest.mark.parametrize("name", list(hh.FORMS))
def test_scripted_sequence_has_every_transition(name):
    w = hh.world(name)
    seq = hh.scripted_sequence(w)
    labels = {label.split()[0] for label, _ in seq}
    assert {f"T{i}" for i in range(1, 13)} <= labels
    by = {label: call for label, call in seq}
    assert hh.work(by["T1 large filtered batch"]) == 40 * 64 and by["T2 peeled batch"].K == 200
    assert by["T12 the first call again"] == by["T1 large filtered batch"] == seq[0][1]
    # every entry is followed by the small probe, then the larger one
    p1, p2 = hh.probes(w)
    assert (p1.B, p1.K, (p1.frm, p1.until)) == (3, 1, vr.sub_range(w.n)) and (p2.B, p2.K, p2.frm, p2.until) == (17, 10, 0, w.n)
    for i in range(0, len(seq), 3):
        assert seq[i][0] != "probe" and [c for _, c in seq[i + 1:i + 3]] == [p1, p2]
    # transition 3: fewer than FILTER_MIN_RB row blocks, a block cut at both ends
    t3 = by["T3 exact scan of a short range"]
    assert (t3.until + 63) // 64 - t3.frm // 64 < hh.TUNE["GULON_FILTER_MIN_RB"]
    assert t3.frm % 64 and t3.until % 64 and t3.until <= w.n
    t4 = [c for label, c in seq if label.startswith("T4")]
    assert any(c.frm == c.until for c in t4) and any(c.K == 0 for c in t4) and any(c.B == 0 for c in t4)
    assert by["T9 partial, K + 1 = 64"].K + 1 == 64
    tuned = [c.arg for _, c in seq if c.kind == "tuning"]
    assert tuned.index(("GULON_FILTER_CAP", 128)) < tuned.index(("GULON_FILTER_CAP", 32768))
    assert ("GULON_SCAN_FILTER", 0) in tuned and tuned[-1] == ("GULON_FILTER_CAP", 32768)
    assert {("GULON_FILTER_NADD", v) for v in (0, 2, 4)} <= set(tuned)
    assert {c.arg for _, c in seq if c.kind == "rejected"} == {"order", "length", "k"}
    assert any(c.kind == "query" and not c.flags for _, c in seq)
    assert {"decode_rows", "query_rows", "query_terms", "bounded", "bounded_dropped"} <= {c.kind for _, c in seq}


@pytest.mark.parametrize("name", list(hh.FORMS))
def test_every_sequence_follows_the_rules(name):
    w = hh.world(name)
    for seq_name, seq in hh.sequences(w).items():
        calls = [c for _, c in seq]
        for i, call in enumerate(calls):
            if call.kind in ("bounded_dropped", "rejected"):            # ... are followed by a valid call
                assert calls[i + 1].kind in hh.QUERY_LIKE and calls[i + 1].kind != "bounded_dropped", (seq_name, i)
            if call.kind == "rejected":
                assert call.frm > call.until or call.until > w.n or call.K > hh.MAX_K_PEELED
            elif call.kind in hh.QUERY_LIKE:
                assert 0 <= call.frm <= call.until <= w.n and hh.depth_of(call) <= hh.MAX_K_PEELED
        if seq_name == "scripted":
            continue
        assert len(seq) == 30 and [i for i, (label, _) in enumerate(seq) if label == "probe"] == list(range(2, 30, 3))
        for probe in hh.probes(w):
            before = [calls[i - 1] for i in range(1, len(calls)) if calls[i] == probe]
            assert any(hh.work(c) > hh.work(probe) for c in before), (seq_name, probe)
            assert any(c.kind in hh.QUERY_LIKE and c.K > probe.K for c in before), (seq_name, probe)


def test_the_view_world_is_the_gathered_index():
    w = hh.world("m16")
    rows = hh.view_rows(w)
    assert np.all(np.diff(rows) > 0) and set(range(0, w.n, 3)) <= set(rows.tolist())
    runs = np.split(rows, np.flatnonzero(np.diff(rows) != 1) + 1)
    assert max(len(r) for r in runs) >= 300
    v = hh.gathered(w, rows, "m16-view")
    assert v.n == len(rows) and np.array_equal(v.idx, w.idx[:, rows])
    for a, b in v.pairs:
        assert np.array_equal(v.idx[:, a], v.idx[:, b])
