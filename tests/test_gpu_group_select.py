"""The grouped index's group selection on its own, against the reference's heap.

Every grouped query starts in coarse_stage (grouped.hip): gq_cdist, then gq_nearest_groups (the literal heap in
registers), or gq_select_groups<8 | 40 | 0> / gq_sorted_groups ((distance, id) sorts that flag what they cannot decide) and
gq_literal_groups (the heap in LDS for the flagged: level 2 at once, level 1 later and only for queries whose result is
redone).  The end-to-end tests compare ten neighbours on random data, where a group wrongly kept or dropped at the cut
almost never shows.  The hook gulon_selftest_group_selection runs the stage alone, as the drivers call it, and returns
nn / nn_cnt / cdist, the flags lit_flag and sel_ok (preset to -1: which kernel wrote them) and nn / nn_cnt again after
the level-1 pass.  tests/group_select_ref.py holds the cases and the plain reference (MathUtils.distanceSq as an fp32 chain,
Index.scala:285-299 on oracle/py_oracle.Heap); test_group_select_ref_host.py asserts without a GPU that the cases hold the
ties they promise.

Per query: (a) cdist bit for bit, NaNs in place; (b) all_literal = 1: count and sequence are the reference's; (c)
all_literal = 0: count and SET are the reference's, the sequence too unless lit = 1, where it is the (distance, id) order
and becomes the reference's after the level-1 pass; (d) nothing over-flagged: pairwise distinct finite distances leave
lit in {-1, 0} and every query of the sorting kernels has exactly the level their rule gives (sorted_level), sel_ok = 1
exactly where at most `cap` entries lie at or below the limit-th key, both flags untouched on the gq_nearest_groups path; (e) nn_stride and stride.  Every case prints a `GSELECT` line (run with -s)."""
import ctypes as C

import numpy as np
import pytest

import group_select_ref as gr

pytestmark = pytest.mark.gpu


class Hook:
    def __init__(self):
        from gulon_amd import native as N
        assert N.device_count() >= 1
        L = C.CDLL(N.HOOKS_LIB_PATH)
        p, i = C.c_void_p, C.c_int32
        self._fn = L.gulon_selftest_group_selection
        self._fn.restype = i
        self._fn.argtypes = [p, i, i, i, i, p, p, p, i, p, i, i, i, i, p, p]
        L.gulon_last_error.restype = C.c_char_p
        self._err = L.gulon_last_error

    def run(self, cs, all_literal):
        """a trivial residual quantizer (m = 1, k = 256, every centroid 0) and zero codes: only the groups matter"""
        b, g, d, n = cs.b, cs.g, cs.d, cs.n
        i32, f32 = np.int32, np.float32
        codes, cents = np.zeros(n, np.uint8), np.zeros(256 * d, f32)
        gc, Q = np.ascontiguousarray(cs.centroids, f32), np.ascontiguousarray(cs.queries, f32)
        offsets = cs.offsets if g > 1 else np.zeros(1, i32)
        bufs = [np.full((b, g), -7, i32), np.full(b, -7, i32), np.zeros((b, g), f32), np.full(b, -7, i32), np.full(b, -7, i32),
                np.full((b, g), -7, i32), np.full(b, -7, i32)]
        ptrs = (C.c_void_p * len(bufs))(*[a.ctypes.data for a in bufs])
        info = np.full(4, -7, i32)
        rc = self._fn(codes.ctypes.data, n, d, 1, 256, cents.ctypes.data, gc.ctypes.data, offsets.ctypes.data, g, Q.ctypes.data, b,
                      cs.strategy, cs.limit, all_literal, ptrs, info.ctypes.data)
        if rc not in (0, cs.expect_rc) and b" failed: " in (self._err() or b""):
            pytest.exit(f"device error in gulon_selftest_group_selection: {self._err()!r}", returncode=3)   # nothing more on a faulted GPU
        assert rc == cs.expect_rc, (rc, self._err())
        if rc:
            return None
        out = dict(zip(["nn", "nn_cnt", "cdist", "lit", "sel_ok", "nn2", "nn_cnt2"], bufs))
        stride = int(info[0])
        assert 1 <= stride <= g
        for k in ("nn", "nn2"):
            out[k] = out[k].reshape(-1)[:b * stride].reshape(b, stride)
        out["info"] = info
        return out


@pytest.fixture(scope="module")
def hook():
    return Hook()


def _seq(nn, cnt, q):
    return [int(c) for c in nn[q, :cnt[q]]]


@pytest.mark.parametrize("name", gr.NAMES)
def test_group_selection_equals_reference(hook, name):
    cs = gr.case(name)
    if cs.expect_rc:                                           # the LDS limit: the library's unsupported status
        for all_literal in (0, 1):
            assert hook.run(cs, all_literal) is None
        print(f"GSELECT {name} path={cs.path}: unsupported ({cs.expect_rc})")
        return
    ref = gr.reference(name)
    path, b, g = cs.path, cs.b, cs.g
    cap = gr.select_cap(cs.limit)
    stride = gr.nn_stride(g, cs.strategy, cs.limit, cs.sizes)
    for all_literal in (1, 0):
        out = hook.run(cs, all_literal)
        nn, cnt, lit, ok = out["nn"], out["nn_cnt"], out["lit"], out["sel_ok"]
        if not all_literal:
            levels = {v: int((lit == v).sum()) for v in (-1, 0, 1, 2)}
            print(f"GSELECT {name} path={path} b={b} cap={cap if path.startswith('select') else 0}: lit -1/0/1/2 = "
                  f"{levels[-1]}/{levels[0]}/{levels[1]}/{levels[2]}, sel_ok -1/0/1 = "
                  f"{int((ok == -1).sum())}/{int((ok == 0).sum())}/{int((ok == 1).sum())}, nn_stride {out['info'][0]} stride {out['info'][1]} "
                  f"lit_cap {out['info'][2]}, largest count {int(cnt.max())}")
        # (a) the distances
        assert np.array_equal(out["cdist"].view(np.uint32)[~np.isnan(ref.cdist)], ref.cdist.view(np.uint32)[~np.isnan(ref.cdist)])
        assert np.array_equal(np.isnan(out["cdist"]), np.isnan(ref.cdist))
        # (e) info
        assert out["info"][0] == stride
        assert out["info"][1] == (max(1, int(cnt.max())) if cs.strategy == 1 and stride > 64 else stride)
        assert set(lit.tolist()) <= {-1, 0, 1, 2} and set(ok.tolist()) <= {-1, 0, 1}
        assert (out["info"][2] > 0) == (not all_literal and path != "nearest")
        for q in range(b):
            want, got = ref.space[q], _seq(nn, cnt, q)
            where = f"{name} all_literal={all_literal} query {q}: lit {lit[q]} sel_ok {ok[q]} ties {sorted(ref.tags[q])}"
            if all_literal:                                     # (b)
                assert got == want, where
            else:                                               # (c)
                assert cnt[q] == len(want) and set(got) == set(want), f"{where}: searched {got[:12]}, reference {want[:12]}"
                if lit[q] == 1:
                    assert got == [int(c) for c in ref.order[q][:cnt[q]]], where
                    assert _seq(out["nn2"], out["nn_cnt2"], q) == want, where
                else:
                    assert got == want, where
                    if out["info"][2] > 0:                      # the level-1 pass leaves every other query alone
                        assert _seq(out["nn2"], out["nn_cnt2"], q) == want, where
            # (d) no over-flagging
            if ref.distinct[q]:
                assert lit[q] in (-1, 0), where
            if path == "nearest":
                assert ok[q] == -1 and lit[q] == -1, where
            elif path.startswith("select"):
                assert ok[q] == (1 if ref.at_or_below[q] <= cap else 0), f"{where}: {ref.at_or_below[q]} at or below, cap {cap}"
            else:
                assert ok[q] == -1, where
            if path != "nearest":                               # exactly the level the rule gives: nothing flagged beyond it
                assert lit[q] == gr.sorted_level(ref.cdist[q], cs.sizes, cs.strategy, cs.limit), where
