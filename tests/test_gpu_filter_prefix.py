"""The prefix test of the flat filter's main stage on the key-sorted copy (filter.hip, GULON_FILTER_PREFIX).

With the key on, a row block is first tested on a prefix of its quantizers; lanes that pass append their place in the
sorted copy to a ring per wave, and the full sixteen look-ups run on whole rings of 64 such rows.  Partial sums are
<= full sums, so the stage keeps the same (query, row) pairs, and ids, distances, counts and flags are those of
GULON_FILTER_PREFIX=0 bit for bit -- on the same handle, whatever the switch was before.  Shapes as in
test_gpu_filter_sort.py: 40 000 rows (625 row blocks, just above filter_min_rb), B = 40 (two full 16-query tiles and a
partial one)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import filter_stage_ref as fs
from test_gpu_filter_sort import B, D, K, KC, M, _results, _same, _trained
from test_gpu_filter_stage import SORTED, Hooks
from test_gpu_query import _check, _make
from test_gpu_subset import _filter_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = {"GULON_FILTER_SORT": 1, "GULON_FILTER_CAP": 32768, "GULON_SCAN_FILTER": 1, "GULON_FILTER_PREFIX": 10}
BUILT = (10,)                       # the prefix lengths the library is built with


@pytest.fixture(scope="module")
def g():
    import gulon_amd
    assert gulon_amd.native.device_count() >= 1
    return gulon_amd


@pytest.fixture
def tune(g):
    before = {k: os.environ.get(k) for k in KNOBS}
    yield g.tune_live
    g.tune_live(**KNOBS)
    for k, v in before.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _off_on(tune, ix, Q, frm=0, until=None, k=K, same_redone=True):
    """The handle's answer without the prefix test, with every built length, and without it again; the filter's
    tile statistics (query tiles, tiles redone exactly) of every run.  same_redone=False where sub-queues overflow:
    a sub-queue belongs to a wave, which rows it gets depends on which wave drew which run, so the number of tiles
    redone may differ from run to run with or without the prefix -- every run must redo some."""
    runs = []
    for p in (0,) + BUILT + (0,) + BUILT:
        tune(GULON_FILTER_PREFIX=p)
        runs.append((ix.batch_query_raw(k, Q, frm, until), _filter_stats(ix)))
    for raw, stats in runs[1:]:
        _same(runs[0][0], raw)
        assert stats[0] == runs[0][1][0]
        assert stats[1] == runs[0][1][1] if same_redone else stats[1] > 0
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [B, 17])
def test_ragged_end_and_tail_tile(oracle, g, tune, b):
    """n = 64 * 625 + 37: the last block is ragged and the last ordering window holds two blocks, so the copy ends in
    padding lanes (row id -1) that may pass the prefix test and sit in a ring; b = 40 and 17 leave a partial tile."""
    n = 64 * 625 + 37
    pq, enc, idx, cents, Q = _trained(g, 3, n)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    raw, (tiles, redone) = _off_on(tune, ix, Q[:b])
    assert tiles > 0 and redone == 0
    _check(oracle, _results(g, raw), *oracle.pq_batch_query(idx, D, KC, cents, Q[:b], K))
    ix.close()


@pytest.mark.gpu
def test_ring_never_fills(oracle, g, tune):
    """Every query is one row of a set of 40 near-duplicates (each off by one centroid) in an index of random codes:
    the bound is the distance to the eleventh of them, the near rows of the whole index are those 40 and a few strays --
    fewer than the 64 a ring emits at -- so what passes the prefix test leaves through the flush at the end of a wave's
    last run."""
    n, near = 40000, 40
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=21)
    rng = np.random.default_rng(11)
    idx = idx.copy()
    where = rng.choice(n, near, replace=False)
    idx[:, where] = idx[:, where[:1]]                        # 40 copies of one row's codes ...
    idx[rng.integers(0, M - 2, near), where] ^= 1            # ... each off by one centroid in one of the first quantizers
    coder = pq.coder_factory(n)
    enc2 = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(M)])
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc2)
    Q = np.ascontiguousarray(ix.decode_rows(np.full(B, where[0], np.int32)), np.float32)
    raw, (tiles, redone) = _off_on(tune, ix, Q)
    assert tiles > 0
    _check(oracle, _results(g, raw), *oracle.pq_batch_query(np.ascontiguousarray(idx), D, KC, cents, Q, K))
    ix.close()


@pytest.mark.gpu
def test_ring_fills_several_times_in_one_run(oracle, g, tune):
    """200 copies of one row, and every query is that row: the copies share their sort key, so they fill more than
    three consecutive 64-row blocks of the sorted copy, every lane of which passes the prefix test for every tile --
    a wave's ring fills and is emptied several times inside one run of four blocks."""
    n, dup = 40001, 200
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=5)
    rng = np.random.default_rng(3)
    idx = idx.copy()
    where = rng.choice(n, dup, replace=False)
    idx[:, where] = idx[:, where[:1]]
    coder = pq.coder_factory(n)
    enc2 = g.EncodedMatrix(coder, [coder.build_code(idx[j]) for j in range(M)])
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc2)
    Q = np.ascontiguousarray(ix.decode_rows(np.full(B, where[0], np.int32)), np.float32)
    raw, (tiles, redone) = _off_on(tune, ix, Q)
    assert tiles > 0 and (raw[3] != 0).any()                 # exact ties: the replay ran
    _check(oracle, _results(g, raw), *oracle.pq_batch_query(np.ascontiguousarray(idx), D, KC, cents, Q, K))
    ix.close()


@pytest.mark.gpu
def test_waves_that_see_most_rows_pass_take_whole_blocks(oracle, g, tune):
    """The per-wave fall-back: a wave of which more than a quarter of the rows passed, over eight blocks or more, takes
    its remaining blocks whole (every lane its row, the full test at once).

    300 000 rows and 1024 queries (64 tiles): the main stage is 8 chunks of about 540 row blocks, 34 per wave.  Half of
    the rows are decoys: the codes of row r0 in the ten quantizers of the prefix (0-7, 14, 15), random ones in the other
    six.  Every query is r0 decoded, so a decoy's partial sums are 0 for every query -- it passes the prefix test --
    while its six random entries put it far beyond the bound.  The decoys share their sort key: they are one
    contiguous half of the sorted copy, several whole chunks, whose waves see every row of their first eight blocks
    pass and take the other ~26 whole.  The true neighbours -- r0 and forty rows that differ from it by one centroid in
    one of the other six quantizers, each at a distance of its own -- have the decoys' key and row ids spread among
    theirs, so most of them sit in blocks taken whole: a fall-back that loses or misplaces rows changes the answer.
    (With every lane of a whole-block turn made dead, this test fails.)"""
    n, b = 300000, 1024
    rng = np.random.default_rng(17)
    cents, idx, pq, _ = _make(oracle, g, 64, D, M, KC, seed=31)          # (the code books; the codes are made here)
    idx = rng.integers(0, KC, (M, n)).astype(np.int32)
    r0 = 12345
    prefix_q = list(range(8)) + [14, 15]
    decoys = rng.choice(n, n // 2, replace=False)
    decoys = decoys[decoys != r0]
    idx[np.ix_(prefix_q, decoys)] = idx[prefix_q, r0][:, None]
    near = decoys[:: len(decoys) // 40][:40]                              # spread over the decoys' row ids
    idx[:, near] = idx[:, r0][:, None]
    for i, row in enumerate(near):                                        # a (quantizer, centroid) of its own each
        j = 8 + i % 6
        idx[j, row] = (idx[j, r0] + 1 + i // 6) % KC
    coder = pq.coder_factory(n)
    enc = g.EncodedMatrix(coder, [coder.build_code(np.ascontiguousarray(idx[j])) for j in range(M)])
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    q0 = np.ascontiguousarray(ix.decode_rows(np.array([r0], np.int32)), np.float32)
    Q = np.ascontiguousarray(np.tile(q0, (b, 1)))
    raw, (tiles, redone) = _off_on(tune, ix, Q)
    assert tiles > 0 and redone == 0
    for part in raw:                                                     # one query 1024 times: one answer
        assert (part == part[0]).all()
    oi, od, oc = oracle.pq_batch_query(np.ascontiguousarray(idx), D, KC, cents, Q[:2], K)
    assert set(oi[0, :oc[0]].tolist()) <= set(near.tolist()) | {r0}       # the neighbours are the rows planted
    _check(oracle, _results(g, tuple(part[:2] for part in raw)), oi, od, oc)
    ix.close()


@pytest.mark.gpu
def test_sub_queue_overflow(oracle, g, tune):
    """Uniform codes, random queries and 64-entry sub-queues: tiles overflow, are flagged and redone exactly."""
    n = 40001
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=9)
    Q = np.random.default_rng(4).standard_normal((B, D)).astype(np.float32)
    tune(GULON_FILTER_SORT=1, GULON_FILTER_CAP=64)
    ix = g.PQIndex(pq, enc)
    raw, (tiles, redone) = _off_on(tune, ix, Q, same_redone=False)
    assert tiles > 0 and redone > 0
    _check(oracle, _results(g, raw), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ix.close()


@pytest.mark.gpu
def test_non_finite_bounds(oracle, g, tune):
    """A NaN query, queries whose distances overflow to +inf (no finite bound: the kernel returns at once for a tile
    whose queries all go to the exact scan), and K = 63 on top of them."""
    n = 40001
    cents, idx, pq, enc = _make(oracle, g, n, D, M, KC, seed=13)
    Q = np.random.default_rng(5).standard_normal((B, D)).astype(np.float32)
    Q[1, 3] = np.nan
    Q[16:32, :] = 1e30                                       # a whole tile without a usable bound
    Q[39, 30] = np.inf
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    for k in (K, 63):
        raw, _ = _off_on(tune, ix, Q, k=k)
        oi, od, oc = oracle.pq_batch_query(idx, D, KC, cents, Q, k)
        for q in range(B):
            assert raw[2][q] == oc[q] and raw[0][q, :oc[q]].tolist() == oi[q, :oc[q]].tolist(), q
            e, v = od[q, :oc[q]], raw[1][q, :oc[q]]
            assert np.array_equal(np.isnan(v), np.isnan(e))
            assert np.array_equal(v[~np.isnan(e)].view(np.uint32), e[~np.isnan(e)].view(np.uint32))
    ix.close()


@pytest.mark.gpu
def test_sub_range_is_unaffected(oracle, g, tune):
    """[from, until) cuts blocks and windows: such a query reads the other copies, with or without the key."""
    pq, enc, idx, cents, Q = _trained(g, 3, 40001)
    tune(GULON_FILTER_SORT=1)
    ix = g.PQIndex(pq, enc)
    for frm, until in ((123, 39999), (1, 40001)):
        raw, _ = _off_on(tune, ix, Q, frm, until)
        _check(oracle, _results(g, raw), *oracle.pq_batch_query(idx, D, KC, cents, Q, K, frm, until))
    ix.close()


@pytest.mark.gpu
def test_switching_on_a_live_handle_and_on_a_context(oracle, g, tune):
    from gulon_amd import native as N
    pq, enc, idx, cents, Q = _trained(g, 0, 40000)
    tune(GULON_FILTER_SORT=1, GULON_FILTER_PREFIX=BUILT[0])
    ix = g.PQIndex(pq, enc)
    ctx = ix.context()
    ref = ix.batch_query_raw(K, Q)
    _same(ref, ctx.batch_query_raw(K, Q))
    for v in (0,) + BUILT + (0,) + BUILT:                    # the context alone, between two batches
        N.check(N.lib().gulon_index_tuning(ctx._h, b"GULON_FILTER_PREFIX", v))
        _same(ref, ctx.batch_query_raw(K, Q))
        _same(ref, ix.batch_query_raw(K, Q))
    for v in (0,) + BUILT:                                   # the parent, its context keeping what it has
        N.check(N.lib().gulon_index_tuning(ix._h, b"GULON_FILTER_PREFIX", v))
        _same(ref, ix.batch_query_raw(K, Q))
        _same(ref, ctx.batch_query_raw(K, Q))
    N.check(N.lib().gulon_index_tuning(ix._h, b"GULON_FILTER_PREFIX", 5))      # a length that is not built: ignored
    _same(ref, ix.batch_query_raw(K, Q))
    _check(oracle, _results(g, ref), *oracle.pq_batch_query(idx, D, KC, cents, Q, K))
    ctx.close()
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["tight", "mixed"])
def test_the_main_stage_queues_the_same_pairs(oracle, tune, regime):
    """ONE main stage on the key-sorted copy through the stage hook (test_gpu_filter_stage.py), which takes its
    tuning from the environment: the queued rows per query -- the stage's survivor set -- and their number are the
    same with and without the prefix test.  (Which sub-queue a row lands in depends on which wave drew its run.)"""
    assert ("m16", regime) in fs.CASES
    hooks = Hooks()
    ref = fs.reference(oracle, "m16", regime)
    tau = ref.taus(0, ref.n)
    got = []
    for p in (0,) + BUILT:
        tune(GULON_FILTER_PREFIX=p)
        rows, counts, flagged, _, _ = hooks.flat(ref, 0, ref.n, tau, SORTED, 4, fs.CAP, 1)
        assert (counts <= fs.CAP).all()                      # nothing lost: the sets are complete
        got.append((np.sort(rows, axis=1), counts.sum(axis=1), flagged))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)
    assert got[0][1].sum() > 0


def test_prefix_kernels_fit_a_cu_twice():
    """The compiler's resource summary of the prefix instantiations: no scratch, at most 64 vector registers and few
    enough scalar registers for eight waves per SIMD (two 16-wave workgroups per CU)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
           os.path.join(ROOT, "gulon_amd", "csrc", "filter.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    found, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            found.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    for p in BUILT:
        mine = [v for k, v in found.items() if "filter_kernelILi16ELi1ELi16ELi4ELi1ELi3ELi%dEEE" % p in k]
        assert len(mine) == 1, (p, sorted(found))
        r = mine[0]
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["TotalSGPRs"] <= 102 and r["Occupancy"] == 8, r


def test_widening_by_complement_keeps_the_same_rows():
    """The arithmetic of the one-instruction widening that scripts/micro/mqsad_rate.hip measures (and the kernel does
    not use: the instruction is too slow): accumulating 255 - byte over the byte-sum groups and testing
    acc >= 255 * groups - QL keeps exactly the rows that sum <= QL keeps -- every byte value, every group count the
    kernel forms (16 quantizers in groups of 4 or 2, the prefix's 3), 16-bit accumulators that never wrap."""
    byte = np.arange(256, dtype=np.int64)
    for nadd in (4, 2):
        ql = 255 // nadd - 1
        for groups in (1, 2, 3, 16 // nadd):
            grid = np.stack(np.meshgrid(*([byte[::17 if groups > 2 else 1]] * min(groups, 3)), indexing="ij"), -1)
            grid = grid.reshape(-1, grid.shape[-1])
            if groups > 3:                                               # the further groups: every byte value, in turn
                grid = np.concatenate([np.concatenate([grid, np.full((len(grid), groups - 3), v)], 1) for v in (0, 1, ql, 255)])
            total = grid.sum(axis=1)
            acc = (255 - grid).sum(axis=1)
            assert acc.max() < 1 << 16 and acc.min() >= 0
            assert np.array_equal(total <= ql, acc >= 255 * groups - ql)

