"""Helpers of test_gpu_stream_contract.py: the two promises include/gulon_hip.h makes about a `void *stream` parameter.

Stream promise -- the work of a call is enqueued on `stream` -- is tested by kind A (run_behind_delay): the stream is
kept busy, the real inputs are copied into the call's buffers BEHIND that delay, and the outputs are read back on the
same stream.  Work put on any other stream (the null stream included: torch's streams do not block against it) runs at
once, on the decoy the buffers still hold, and returns the decoy's answer.

Handle promise -- device work of consecutive calls on one handle is ordered, whatever their streams -- is tested by
kind B (run_two_streams): call X waits behind a delay on stream A, call Y goes to stream B at once; Y's device work
may only finish after the delay has.

Nothing here synchronises between enqueueing the delay and the final stream synchronise except where it says so."""
import ctypes as C
import os
import re
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gulon_hip.h")

I_FILL, F_FILL = -7777, -7777.0        # sentinels of the output buffers
MIN_DELAY_MS, MAX_DELAY_MS, DELAY_FACTOR = 50.0, 500.0, 20.0


# ---------------------------------------------------------------- the header
def header_text():
    with open(HEADER) as f:
        return f.read()


def stream_entry_points(text):
    """Every function the header declares with a `void *stream` parameter (comments and #ifdef'd hooks included:
    a declaration is a declaration)."""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = set()
    for m in re.finditer(r"\bint(?:32|64)_t\s+(gulon_\w+)\s*\(([^;{}]*)\)\s*;", code):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            names.add(m.group(1))
    return names


def device_pointer_entry_points_without_stream(text):
    """Functions with a `d_` pointer parameter (or a `_dev` name) and no stream parameter."""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = set()
    for m in re.finditer(r"\bint(?:32|64)_t\s+(gulon_\w+)\s*\(([^;{}]*)\)\s*;", code):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            continue
        if m.group(1).endswith("_dev") or re.search(r"\*\s*\*?\s*d_\w+", m.group(2)):
            names.add(m.group(1))
    return names


def comments_naming(text, name):
    return [c for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if re.search(r"\b%s\b" % re.escape(name), c)]


# ---------------------------------------------------------------- a delay on a stream
class Delay:
    """busy(stream, ms): device work of about `ms` milliseconds on `stream`, calibrated once with timing events."""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:                                     # a chain of large device-to-device copies
            self.a = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
            self.b = torch.empty_like(self.a)
        self.unit = 100_000 if self.sleep else 1                   # cycles / copies per calibration step
        self._step(self.unit)                                      # (loads the kernel)
        while True:
            ms = self._timed(self.unit)
            if ms >= 2.0 or self.unit >= 10 ** 12:
                break
            self.unit *= 8
        self.units_per_ms = self.unit / max(ms, 1e-3)

    def _step(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.b.copy_(self.a, non_blocking=True)

    def _timed(self, units):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self._step(units)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def busy(self, stream, ms):
        with self.torch.cuda.stream(stream):
            self._step(max(1, int(ms * self.units_per_ms)))


def delay_ms_for(return_seconds):
    """max(20 x the warm call's host return time, 50 ms), capped at 500 ms"""
    return min(max(DELAY_FACTOR * return_seconds * 1e3, MIN_DELAY_MS), MAX_DELAY_MS)


# ---------------------------------------------------------------- a case
class Handle:
    """What a case calls: .h (the C handle or None), anything else by attribute; close() closes `keep` in order."""

    def __init__(self, h=None, keep=(), **more):
        self.h, self.keep = h, list(keep)
        self.__dict__.update(more)

    def close(self):
        for o in self.keep:
            o.close()
        self.keep = []


@dataclass
class Case:
    name: str
    entries: Tuple[str, ...]                       # the entry point(s) of the header this case calls with the stream
    make: Callable[[], Handle]                     # a FRESH handle of the same build
    ins: Dict[str, Tuple[np.ndarray, np.ndarray]]  # device inputs: (real, decoy), same shape and type
    outs: Dict[str, Tuple[tuple, type, float]]     # device outputs: (shape, dtype, initial fill)
    call: Callable                                 # (H, p: name -> device address, st: c_void_p or None, host: dict) -> status
    host: Optional[Callable] = None                # (H, real inputs) -> outputs of the host-pointer form
    syncs: bool = False                            # the header says the call synchronises (or may synchronise) `stream`
    waits: bool = False                            # this case's path reads back on the stream: the call must wait for it
    inout: Tuple[str, ...] = ()                    # inputs the call overwrites: read back as outputs
    scratch: Dict[str, Tuple[tuple, type]] = field(default_factory=dict)   # device buffers between two calls, not compared
    status: Optional[Callable] = None              # (H) -> the handle's status word, read after the stream
    spoil: Optional[Callable] = None               # (real inputs) -> the same with exactly one offending id
    defined: Optional[Callable] = None             # (outputs) -> outputs with what the header leaves undefined masked
    check_ref: Optional[Callable] = None           # (H, reference outputs): the path this case is named after was taken

    def inputs(self, which, bad=False):
        d = {k: np.ascontiguousarray(v[which]) for k, v in self.ins.items()}
        return self.spoil(d) if (bad and which == 0) else d


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differs(x, y):
    return any(not same_bits(x[k], y[k]) for k in x)


def assert_same(got, want, what):
    assert set(got) >= set(want), (what, sorted(got), sorted(want))
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if not same_bits(a, b):
            if a.shape != b.shape or a.dtype != b.dtype:
                raise AssertionError(f"{what}: output {k!r}: {a.dtype}{a.shape} against {b.dtype}{b.shape}")
            bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)) // a.dtype.itemsize
            i = int(bad[0])
            raise AssertionError(f"{what}: output {k!r} differs in {len(np.unique(bad))} of {a.size} entries; first at "
                                 f"{i}: {a.reshape(-1)[i]!r} against {b.reshape(-1)[i]!r}")


class Buffers:
    """The device side of one call: inputs, outputs (filled with their sentinel), scratch."""

    def __init__(self, torch, case, inputs):
        self.torch, self.case = torch, case
        self.ins = {k: torch.from_numpy(v.copy()).to("cuda") for k, v in inputs.items()}
        self.outs = {k: torch.full(shape, fill, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
                     for k, (shape, dt, fill) in case.outs.items()}
        self.scratch = {k: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
                        for k, (shape, dt) in case.scratch.items()}
        self.host = {}

    def ptrs(self):
        p = {k: t.data_ptr() for k, t in self.ins.items()}
        p.update({k: t.data_ptr() for k, t in self.outs.items()})
        p.update({k: t.data_ptr() for k, t in self.scratch.items()})
        return p

    def results(self):
        r = dict(self.outs)
        r.update({k: self.ins[k] for k in self.case.inout})
        return r

    def finish(self, fetched):
        out = {k: v.numpy().copy() for k, v in fetched.items()}
        out.update({"host:" + k: np.array(v) for k, v in self.host.items()})
        return self.case.defined(out) if self.case.defined else out


def stream_arg(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def run_synchronised(torch, case, H, inputs, stream=None):
    """The call with everything synchronised around it -> (status, outputs, status word, seconds the call took to
    return on the host)."""
    bufs = Buffers(torch, case, inputs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = case.call(H, bufs.ptrs(), stream_arg(stream), bufs.host)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    res = bufs.finish({k: t.cpu() for k, t in bufs.results().items()})
    word = case.status(H) if case.status else None
    return rc, res, word, t1 - t0


@dataclass
class BehindDelay:
    rc: int
    outputs: dict
    word: Optional[int]
    pending_at_return: bool
    delay_ms: float
    return_ms: float


def run_behind_delay(torch, delay, case, H, real, decoy, ms):
    """Kind A.  The buffers hold the decoy; on a fresh stream: the delay, event eS, the real inputs copied in, the call,
    the outputs copied out to pinned memory, one stream synchronise."""
    bufs = Buffers(torch, case, decoy)
    staged = {k: torch.from_numpy(v.copy()).to("cuda") for k, v in real.items()}
    res = bufs.results()
    pinned = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in res.items()}
    stream = torch.cuda.Stream()
    eS = torch.cuda.Event()
    torch.cuda.synchronize()                                        # the last one before the stream's own
    delay.busy(stream, ms)
    with torch.cuda.stream(stream):
        eS.record(stream)
        for k, t in bufs.ins.items():
            t.copy_(staged[k], non_blocking=True)
        t0 = time.perf_counter()
        rc = case.call(H, bufs.ptrs(), stream_arg(stream), bufs.host)
        t1 = time.perf_counter()
        pending = not eS.query()
        for k, t in res.items():
            pinned[k].copy_(t, non_blocking=True)
    stream.synchronize()
    word = case.status(H) if case.status else None
    return BehindDelay(rc, bufs.finish(pinned), word, pending, ms, (t1 - t0) * 1e3)


# ---------------------------------------------------------------- two streams
def independent_streams(torch, delay, tries=8):
    """Two streams whose work overlaps on this device: while A sleeps, a trivial operation on B finishes.  Streams
    that share a hardware queue run one after the other and would let a handle without any ordering pass."""
    A = torch.cuda.Stream()
    x = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(tries - 1):
        B = torch.cuda.Stream()
        eS, eB = torch.cuda.Event(), torch.cuda.Event()
        delay.busy(A, MIN_DELAY_MS)
        eS.record(A)
        with torch.cuda.stream(B):
            x.add_(1.0)
            eB.record(B)
        eB.synchronize()
        overlapped = not eS.query()
        A.synchronize()
        if overlapped:
            return A, B
    return None


@dataclass
class TwoStreams:
    rc: Tuple[int, int]
    outputs: Tuple[dict, dict]
    y_returned_pending: bool       # Y's call came back to the host while A's delay was still pending
    ordered: bool                  # Y's device work finished after A's delay: it waited for X
    delay_ms: float


def run_two_streams(torch, delay, X, Y, H, x_in, y_in, A, B, ms):
    """Kind B.  On A: the delay, eS, X; on B, at once: Y, eB.  eB.synchronize(); then eS must have happened."""
    bx, by = Buffers(torch, X, x_in), Buffers(torch, Y, y_in)
    eS, eB = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    delay.busy(A, ms)
    eS.record(A)
    rcx = X.call(H, bx.ptrs(), stream_arg(A), bx.host)
    rcy = Y.call(H, by.ptrs(), stream_arg(B), by.host)
    y_pending = not eS.query()
    eB.record(B)
    eB.synchronize()
    ordered = eS.query()
    A.synchronize()
    B.synchronize()
    torch.cuda.synchronize()
    ox = bx.finish({k: t.cpu() for k, t in bx.results().items()})
    oy = by.finish({k: t.cpu() for k, t in by.results().items()})
    return TwoStreams((rcx, rcy), (ox, oy), y_pending, ordered, ms)
