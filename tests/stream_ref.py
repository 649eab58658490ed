"""The streaming receiver of ofdm_stream_push (include/ofdm_hip.h, "a streaming receiver") without a GPU, shared by
tests/test_stream_cpu.py and tests/test_gpu_stream.py.

Notation: T samples pushed so far, L = S, W = reps L, b = sync_backoff, valid = T - W - L + 1, H = W + (10 + max_symbols) S + 2.

  * deliveries: THE DEFINITION.  The whole-stream scan (scan_ref.scan, lag_lo = 0) and packets_ref.packets on the whole capture, shared out
    over the pushes by the horizon rule: packet k belongs to the first push after which T >= d1_k + H, or to the flush;
  * Window: a literal model of the library's host logic.  It keeps only the retained samples, runs scan_ref.scan on the window from the lag
    the walk resumes at, commits by the horizon rule, decodes with window-relative timing and re-bases.  It must reproduce `deliveries`
    for every partition (tests/test_stream_cpu.py): that is the argument that the library's bookkeeping loses and doubles nothing;
  * horizon / retained_from / window_bound: the three integer rules both use;
  * cuts_*: the partitions of the tests.
"""
from collections import namedtuple

import numpy as np

import packets_ref as P
import scan_ref as R

ALL = 10 ** 9


def horizon(S, reps, max_symbols):
    return reps * S + (10 + max_symbols) * S + 2


def window_bound(S, reps, max_symbols, backoff, max_chunk):
    """the most samples a window ever holds"""
    return horizon(S, reps, max_symbols) + S + backoff + 2 + max_chunk


def retained_from(lo, S, backoff, B, T):
    """the first sample the window keeps once the walk resumes at lag lo: (lo - L - b) & ~1 clamped to what the window holds, [B, T]"""
    return max(min(max(lo - S - backoff, B), T) & ~1, B)


def ends_of(sizes):
    """push sizes -> T after every push"""
    return np.cumsum(np.asarray(sizes, np.int64)).tolist()


def share(d1, H, ends, flush=True):
    """-> per push the indices k of the packets it delivers: the first push after which T >= d1_k + H; with flush the last push takes the rest"""
    out = [[] for _ in ends]
    for k, d in enumerate(d1):
        p = next((i for i, T in enumerate(ends) if T >= d + H), None)
        if p is None and flush:
            p = len(ends) - 1
        if p is not None:
            out[p].append(k)
    return out


Whole = namedtuple("Whole", "scan packets H")


def whole(orc, x32, n_fft, reps, thr, holdoff, guard, mod, max_symbols, backoff=4, cfo_mode=P.CFO_SIGNED, training=None, sums=None):
    """A(T) for T = the whole capture: the scan and every packet of it"""
    S = n_fft + n_fft // 4
    sc = R.scan(orc, x32, S, reps, thr, holdoff, ALL, 0, 0, sums=sums)
    pk = P.packets(orc, x32, {"d_hat": sc.d_hat, "f_delta": sc.f_delta, "metric": sc.metric}, n_fft, guard, mod, max_symbols, backoff, cfo_mode, training)
    return Whole(sc, pk, horizon(S, reps, max_symbols))


def deliveries(orc, x32, sizes, n_fft, reps, thr, holdoff, guard, mod, max_symbols, backoff=4, flush=True, w=None, **kw):
    """-> (Whole, per push the list of packet indices).  sizes: the samples of every push (their sum is the capture); w: whole() of the
    capture if the caller has it"""
    w = whole(orc, x32, n_fft, reps, thr, holdoff, guard, mod, max_symbols, backoff, **kw) if w is None else w
    assert sum(sizes) == len(x32)
    return w, share(w.scan.d1, w.H, ends_of(sizes), flush)


# ---------------------------------------------------------------- the library's host logic, literally
class Window:
    """ofdm_stream on numpy arrays.  push() -> the packets this push delivers, as dicts with stream-relative d1, d_hat, offset"""

    def __init__(self, orc, n_fft, reps, thr, holdoff, guard, mod, max_symbols, backoff=4, max_chunk=1 << 40, scan_cap=256, first_sample=0):
        self.orc, self.n_fft, self.reps, self.thr, self.holdoff = orc, n_fft, reps, thr, holdoff
        self.guard, self.mod, self.D, self.b, self.max_chunk, self.cap, self.first = guard, mod, max_symbols, backoff, max_chunk, scan_cap, first_sample
        self.S = n_fft + n_fft // 4
        self.W = reps * self.S
        self.H = horizon(self.S, reps, max_symbols)
        self.x = np.zeros(0, np.complex64)          # the window: samples [B, T)
        self.T = self.B = self.keep_from = self.lo = 0
        self.ended = False
        self.max_window = 0

    def _piece(self, chunk, flush):
        out = []
        if len(chunk):
            self.x = np.concatenate([self.x[self.keep_from - self.B:], chunk])      # the ingest: the carry, then the chunk
            self.B = self.keep_from
            self.T += len(chunk)
            self.max_window = max(self.max_window, len(self.x))
        assert self.B % 2 == 0 and len(self.x) == self.T - self.B
        valid = self.T - self.W - self.S + 1
        while valid > 0 and self.lo < valid:
            sc = R.scan(self.orc, self.x, self.S, self.reps, self.thr, self.holdoff, self.cap, self.lo - self.B, 0)
            nc = 0
            while nc < len(sc.d1) and (flush or self.B + sc.d1[nc] + self.H <= self.T):
                nc += 1
            for k in range(nc):
                p = P.packet(self.orc, self.x, sc.d_hat[k], sc.f_delta[k], sc.metric[k], self.n_fft, self.guard, self.mod, self.D, self.b)
                base = self.B + self.first
                p.update(d1=base + sc.d1[k], d_hat=base + sc.d_hat[k], offset=base + p["offset"], scan_f_delta=sc.f_delta[k])
                out.append(p)
            if nc < len(sc.d1):                      # deferred: the first crossing at or after it is itself
                self.lo = self.B + sc.d1[nc]
                break
            if sc.d1:
                self.lo = self.B + sc.d1[-1] + self.holdoff
            if not sc.more:
                self.lo = max(self.lo, valid)
                break
        self.keep_from = retained_from(self.lo, self.S, self.b, self.B, self.T)
        return out

    def push(self, chunk, flush=False):
        assert not self.ended
        chunk = np.asarray(chunk, np.complex64).reshape(-1)
        out, done = [], 0
        if len(chunk) == 0 and not flush:
            return out
        while True:
            m = min(len(chunk) - done, self.max_chunk)
            out += self._piece(chunk[done: done + m], flush and done + m == len(chunk))
            done += m
            if done >= len(chunk):
                break
        self.ended = bool(flush)
        return out


# ---------------------------------------------------------------- partitions (push sizes that sum to n)
def cuts_equal(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def cuts_at(n, *at):
    """one cut at every given sample index inside (0, n)"""
    edges = sorted({a for a in at if 0 < a < n})
    return [b - a for a, b in zip([0] + edges, edges + [n])]


def cuts_edges(n, d1, d_hat, H, S, backoff):
    """the four edge cuts of one detection: at d1 + 1, d1 + H - 1, d1 + H and r + 1 (r its row start)"""
    r = max(d_hat - S - backoff, 0) & ~1
    return cuts_at(n, d1 + 1, d1 + H - 1, d1 + H, r + 1)


def cuts_random(n, seed, lo=1, hi=10_000):
    rng = np.random.default_rng(seed)
    sizes, left = [], n
    while left > 0:
        m = int(min(left, rng.integers(lo, hi + 1)))
        sizes.append(m)
        left -= m
    return sizes
