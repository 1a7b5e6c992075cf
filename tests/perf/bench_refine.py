"""Refined-query benchmark at the headline shape (10 M x 128, m = 16, k = 256, batch 1024, k_nn = 10, c = 100): what the
exact re-ranking stage (csrc/refine.hip) costs next to the scan that feeds it and to the existing kernel that does the
same gather and arithmetic without the selection, and what it buys in recall.  Timed, not gated.
   python tests/perf/bench_refine.py [rows] [dim] [k_nn] [candidates]
Every time is the median of BLOCKS blocks of STEPS back-to-back steps, after warm-up, the device idle before a block."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import gulon_amd as g
from gulon_amd import native as N
from gulon_amd import tests_recall as tr
from gulon_amd.recall import sample_rows

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
c = int(sys.argv[4]) if len(sys.argv) > 4 else 100
m, k, B, iters = 16, 256, 1024, 10
WARMUP, BLOCKS, STEPS = 3, 7, 10
L = N.lib()
dm = g.DeviceMatrix.synthetic(n, d, 3, 1234, 1000)
pq = g.ProductQuantizer.apply(dm, g.ProductQuantizerConfig(k, m, iters))
index = g.Index.sorted(dm, pq)
h = index.vector_index._h
Qh = dm.get_rows(sample_rows(n, B, 0))
Q = torch.from_numpy(Qh).cuda()


def buffers(width):
    return (torch.empty((B, width), dtype=torch.int32, device="cuda"),
            torch.empty((B, width), dtype=torch.float32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))


ci, cd, cc = buffers(c)
cf = torch.empty(B, dtype=torch.int32, device="cuda")
oi, od, oc = buffers(K)


def scan():                                                   # (a) batch_query(k = c): the candidates
    N.check(L.gulon_index_batch_query_dev(h, Q.data_ptr(), B, c, 0, n, ci.data_ptr(), cd.data_ptr(), cc.data_ptr(),
                                          cf.data_ptr(), None))


def refine():                                                 # (c) the refine stage alone, over those candidates
    N.check(L.gulon_refine_topk_dev(dm._h, Q.data_ptr(), B, ci.data_ptr(), c, None, 0, K, oi.data_ptr(), od.data_ptr(),
                                    oc.data_ptr(), None))


def both():
    scan()
    refine()


scan()
torch.cuda.synchronize()
cand = ci.cpu().numpy()
ks, cut = np.asarray([c], np.int32), np.zeros((B, 1), np.float32)


def gather_only():                                            # (b) gulon_recall_counts with out_dist: host form, so its
    tr.recall_counts(dm, Qh, cand, ks, cut, distances=True)   #     time includes the copies of B x c rows and distances


def refine_host():                                            # (c'), the like-for-like of (b): the host form of the stage
    g.refine_topk(dm, Qh, cand, K)


def timed(step):
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(BLOCKS):
        t = time.perf_counter()
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t) / STEPS * 1e3)
    return {"median_ms": statistics.median(blocks), "min_ms": min(blocks), "max_ms": max(blocks)}


times = {"a_scan_k_eq_c": timed(scan), "b_recall_counts_host": timed(gather_only), "c_refine_stage_dev": timed(refine),
         "c_refine_stage_host": timed(refine_host), "c_refined_query_end_to_end": timed(both)}

# recall before and after: Tests.recall_of on the bench data, the sampled rows as queries.  Index rows ARE the vectors'
# rows here, so the "words" are the row numbers themselves (ten million strings and their key index would only cost time)
class _Rows:
    def __getitem__(self, i):
        return i

    @staticmethod
    def lookup(word):
        return word


class _Vectors:
    matrix, key_index, size = dm, _Rows, n


class _Plain:
    words, size = _Rows(), n

    def batch_query_raw(self, kk, q):
        oi_, od_, oc_, of_ = index.vector_index.batch_query_raw(kk, q)
        return np.where(np.arange(kk)[None, :] < oc_[:, None], oi_, -1), od_, oc_, of_


class _Refined(_Plain):
    def batch_query_raw(self, kk, q):
        cand_, _, _, of_ = _Plain.batch_query_raw(self, max(c, kk), q)
        return g.refine_topk(dm, q, cand_, kk) + (of_,)


tests = tr.Tests.for_queries(_Vectors, Qh, ks=(1, K))
plain, after = tests.recall_of(_Plain()), tests.recall_of(_Refined())
print(json.dumps({"metric": "refine_stage_ms", "value": times["c_refine_stage_dev"]["median_ms"], "unit": "ms",
                  "config": {"workload": f"SortedIndex {n}x{d}, PQ(m={m},k={k}), batch={B}, K={K}, candidates={c}",
                             "warmup": WARMUP, "blocks": BLOCKS, "steps_per_block": STEPS},
                  "times": times,
                  "recall": {f"plain_R@{kk}": float(plain[kk].mean) for kk in sorted(plain)} |
                            {f"refined_R@{kk}": float(after[kk].mean) for kk in sorted(after)}}), flush=True)
