"""The grouped index's pre-selection on its own, against float64: what gq_rerank's certificate rests on.

Nothing in grouped_filter.hip or gq_approx_scan is the reference's arithmetic: these kernels choose 64 candidates per
query, and gq_rerank certifies an answer with `ek < a_last - margin`.  That holds only while the list IS the 64 smallest
(D~, row) of every searched row and |D~ - D| <= margin -- and a pre-selection that flags everything passes every
end-to-end test, because the literal kernels then give the reference's answer.  The test hook
gulon_selftest_grouped_stage (grouped.hip) builds a grouped index, runs coarse_stage and then the pre-selection BOTH ways on
the same nn lists (group_filter_run; gq_ptables + gq_approx_scan + merge), gq_rerank on each list, and returns every
intermediate: the per-index state, the per-query tables, budgets and 8-bit levels, the tiles, the queued (row, base)
pairs, both lists with their flags, both answers with their redo lists.  tests/grouped_stage_ref.py holds the cases,
the float64 reference, the derivation of every bound and the checks; its preconditions are asserted without a GPU in
test_oracle_cross.py.  DESIGN.md 9p lists the kernel instantiation each case runs.

Base shape: n = 9037, B = 37, g = 48, LimitGroups(20), S = 10, K = 10, m16 k256 d32; a case differs from it in what its name
says.  Every case prints a `GSTAGE` line (run with -s): the largest rows queued / rows that must be kept / upper set
over the queries that filter, the largest |lv - D| / E, and the queries certified by each path."""
import ctypes as C

import numpy as np
import pytest

import grouped_stage_ref as gs

pytestmark = pytest.mark.gpu

REFUSED = 78


class Hook:
    def __init__(self):
        import gulon_amd
        from gulon_amd import native as N
        assert N.device_count() >= 1
        self.g = gulon_amd
        L = C.CDLL(N.HOOKS_LIB_PATH)
        p, i = C.c_void_p, C.c_int32
        self._fn = L.gulon_selftest_grouped_stage
        self._fn.restype = i
        self._fn.argtypes = [p, i, i, i, i, p, p, p, i, p, i, i, i, i, p, p]
        L.gulon_last_error.restype = C.c_char_p
        self._err = L.gulon_last_error

    def run(self, cs, limit=None, expect=0):
        if getattr(cs, "packed", None) is None:
            cs.packed = cs.pack(self.g)
        n, b, g, kk, mp = cs.n, cs.b, cs.g, cs.kk, cs.m_pad
        limit = cs.limit if limit is None else limit
        room = b * g // gs.GF_QT + g + 1
        i32, f32, u8 = np.int32, np.float32, np.uint8
        bufs = [np.full((b, g), -7, i32), np.full(b, -7, i32), np.zeros((b, g), f32), np.zeros(n, f32), np.zeros(g, f32),
                np.full(-(-n // 64) * 64, 0xEE, u8), np.zeros(g, f32), np.zeros(4, f32), np.zeros((b, mp, 256), f32),
                np.zeros((b, 4), f32), np.full((b, gs.GF_NT, 256), 0xEE, u8), np.full(g, -7, i32), np.full((room, 24), -7, i32),
                np.full(4, -7, i32), np.full(b, -7, i32), np.zeros((b, gs.GF_CAP, 2), np.uint32)]
        for _ in range(2):
            bufs += [np.zeros((b, 64), f32), np.full((b, 64), -7, i32), np.full((b, 16), -7, i32)]
        for _ in range(2):
            bufs += [np.full((b, kk), -7, i32), np.zeros((b, kk), f32), np.full(b, -7, i32), np.full(1, -7, i32), np.full(b, -7, i32)]
        ptrs = (C.c_void_p * len(bufs))(*[a.ctypes.data for a in bufs])
        info = np.full(8, -7, i32)
        offsets = cs.offsets if len(cs.offsets) else np.zeros(1, i32)
        rc = self._fn(cs.packed.ctypes.data, n, cs.d, cs.m, cs.k, cs.cents.ctypes.data, cs.gcent.ctypes.data, offsets.ctypes.data, g,
                      cs.Q.ctypes.data, b, kk, cs.strategy, limit, ptrs, info.ctypes.data)
        if rc not in (0, expect) and b" failed: " in (self._err() or b""):
            pytest.exit(f"device error in gulon_selftest_grouped_stage: {self._err()!r}", returncode=3)   # nothing more on a faulted GPU
        assert rc == expect, (rc, self._err())
        if expect:
            return None
        stride = int(info[0])
        assert info[1] == mp and info[4] == gs.GF_CAP and info[5] == gs.GF_PLACED
        names = ["nn", "nn_cnt", "cdist", "xnorm", "xnlo", "xcode", "gnorm", "scalars", "P", "qs", "qb", "gcnt", "tiles", "meta", "qcnt",
                 "queue", "amv0", "ami0", "anan0", "amv1", "ami1", "anan1", "oi0", "od0", "oc0", "nredo0", "redo0", "oi1", "od1",
                 "oc1", "nredo1", "redo1"]
        out = dict(zip(names, bufs))
        out["nn"] = out["nn"].reshape(-1)[:b * stride].reshape(b, stride)
        out["tiles"] = out["tiles"][:max(int(out["meta"][0]), 0)]
        out["info"] = info
        return out


@pytest.fixture(scope="module")
def hook():
    return Hook()


def _run(oracle, hook, name):
    cs = gs.case(oracle, name)
    with np.errstate(all="ignore"):
        out = hook.run(cs)
        stats, worst, certified, edges = gs.check_stage(cs, out, oracle)
    filt = np.array([s for q, s in enumerate(stats) if out["qs"][q, 1] != 0] or [(0, 0, 0)])
    print(f"GSTAGE {name} vec={out['info'][2]} ng={out['info'][3]} tiles={out['meta'][0]} pairs={out['meta'][1]}: queued/must keep/upper set "
          f"{'/'.join(str(v) for v in filt.max(axis=0))}, keep-all queries {int((out['qs'][:, 1] == 0).sum())}, largest |lv - D| / E {worst:.4f}, "
          f"certified {certified[0]} by group / {certified[1]} by scan of {cs.b}, {edges} on the edge")
    return cs, out, stats, certified


# (VEC, code words) of every case: the instantiation DESIGN.md 9p names
SHAPE = {"m8": (4, 2), "m5": (4, 2), "m12": (4, 3), "m3": (4, 1), "d128": (4, 2), "d129": (4, 2), "d200": (4, 2), "d5": (4, 2)}


@pytest.mark.parametrize("name", [c for c in gs.REGULAR if c not in gs.LOOSE])
def test_preselection_keeps_and_lists_the_right_rows(oracle, hook, name):
    cs, out, stats, certified = _run(oracle, hook, name)
    assert (int(out["info"][2]), int(out["info"][3])) == SHAPE.get(name, (16, 1))
    assert (out["qs"][:, 1] != 0).all(), "every query of a regular case filters"
    for q, (queued, must, upper) in enumerate(stats):                 # the preconditions, on the device's own figures
        assert queued <= upper < gs.GF_CAP, (name, q, queued, must, upper)
    # a pre-selection that flags or redoes everything passes every end-to-end test: here it must certify (K = 63: ek IS the 64th)
    assert name == "k63" or min(certified) * 2 >= cs.b, (name, "certified", certified)
    if name == "g90":
        assert out["meta"][0] > 64 and (out["gcnt"][[0, 17, 18, 63]] == 0).all()       # gf_tiles over two workgroups, empty groups
    if name == "big_group":
        assert (out["qcnt"][::3] > 0).all() and cs.sizes[gs.BIG_GROUP] == 2500
    if name in ("b16", "b17", "b1"):
        nq = sorted(int(t[1]) for t in out["tiles"] if t[0] == gs.BIG_GROUP)
        assert nq == {"b16": [16], "b17": [1, 16], "b1": [1]}[name], nq
    if name == "vectors1500":
        assert len(set(out["nn_cnt"].tolist())) > 1 and out["nn_cnt"].max() < out["nn"].shape[1]


def test_shifted_centroids_strain_the_margin(oracle, hook):
    """|g| ~ 1000, |r| ~ 1: qq - 2 qg + xnorm cancels six digits.  One norm level swallows a group (LOOSE: no tightness to
    speak of), every other check holds -- |lv - D| <= E above all."""
    _run(oracle, hook, "shifted")


def test_small_groups_list_nearly_every_searched_row(oracle, hook):
    """~8 rows per group, LimitGroups(17): the sample spans 16 groups without reaching 256 rows, and 64 of a query's ~136
    searched rows are listed, so the margin check sees nearly every pair."""
    cs, out, stats, certified = _run(oracle, hook, "rows8")
    assert (out["qs"][:, 1] != 0).sum() * 2 >= cs.b


def test_fewer_than_64_searched_rows_keep_everything(oracle, hook):
    """~3 rows per group: tq = inf, 1 / step = 0, every searched row queued, lists padded, ncand < 64 in gq_rerank"""
    cs, out, stats, certified = _run(oracle, hook, "rows3")
    short = [q for q in range(cs.b) if len(cs.searched(out["nn"], out["nn_cnt"], q)) < 64]
    assert len(short) * 2 >= cs.b and (out["qs"][short, 1] == 0).all()
    assert all((out["ami0"][q] == gs.INT_MAX).any() for q in short) and min(certified) * 2 >= cs.b


@pytest.mark.parametrize("name", ["nan", "inf", "huge"])
def test_non_finite_queries_keep_everything_and_are_redone(oracle, hook, name):
    """Query 3 has a NaN coordinate / an inf coordinate / is scaled by 1e20 (|q|^2 overflows): 1 / step = 0, every searched
    row queued, the query redone by both paths; the other 36 queries are filtered and certified as ever."""
    cs, out, stats, certified = _run(oracle, hook, name)
    assert out["qs"][3, 1] == 0 and all(3 in out["redo%d" % p][:out["nredo%d" % p][0]] for p in range(2))
    assert (np.delete(out["qs"][:, 1], 3) != 0).all() and min(certified) * 2 >= cs.b
    if name == "nan":
        assert out["anan0"][3, 0] == 1 and out["anan1"][3].any()


def test_more_ties_at_the_cut_than_the_placing_holds(oracle, hook):
    """600 copies of one row, every third query at it: 600 > GF_PLACED entries at the 64th smallest D~ -- flagged"""
    cs, out, stats, certified = _run(oracle, hook, "copies600")
    assert (out["anan0"][::3, 0] == 1).all() and (out["qcnt"][::3] >= 600).all() and (out["qcnt"] <= gs.GF_CAP).all()
    assert not np.delete(out["anan0"][:, 0], np.arange(0, cs.b, 3)).any()


def test_overflowing_queue_is_clamped_and_flagged(oracle, hook):
    """n = 20000 with 17000 copies of one row: the queues of the queries at it hold GF_CAP entries of more than GF_CAP
    counted, every one a searched row (check_queue), and the queries are flagged"""
    cs, out, stats, certified = _run(oracle, hook, "copies17000")
    assert (out["qcnt"][::3] >= 17000).all() and (out["anan0"][::3, 0] == 1).all()
    assert (np.delete(out["qcnt"], np.arange(0, cs.b, 3)) < gs.GF_CAP).all()


def test_hook_refuses_what_the_driver_would_not_send_by_group(oracle, hook):
    """LimitGroups(16) is at most GF_SAMPLE_GROUPS groups: run_grouped_query takes gq_approx_scan, the hook answers 78"""
    hook.run(gs.case(oracle, "m16"), limit=16, expect=REFUSED)
