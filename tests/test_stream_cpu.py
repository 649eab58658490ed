"""The streaming receiver (EXT-14, include/ofdm_hip.h "a streaming receiver") without a GPU: the integer facts the contract rests on, the
model of the host logic against the definition (tests/stream_ref.py), and the surface.

  1. the horizon: a detection committed at T (d1 + H <= T) has its whole peak window below valid and its whole gathered row inside the
     stream, so every field of its packet is the same at every T' >= T -- proved in integers over all reps, backoffs, max_symbols and N;
  2. the retention: the window never exceeds H + L + b + 2 + max_chunk samples, and no later row starts in front of the retained start;
  3. Window == deliveries on the certified captures n64_a and n256 (their decisions have margins: no summation order matters), for one
     push, chunks of 4096 and of 997, and the four edge cuts of one detection;
  4. the new functions stand in the header, the ctypes table, the Rust text and ofdm_host.hpp;
  5. every new function returns OFDM_ERR_INVALID on NULL handles, without a GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packets_ref as P
import scan_ref as R
import stream_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_stream_create", "ofdm_stream_destroy", "ofdm_stream_reset", "ofdm_stream_push", "ofdm_stream_push_sc16", "ofdm_stream_state")


# ---------------------------------------------------------------------------------------------------------- 1: the horizon
@pytest.mark.parametrize("n_fft", (64, 256, 1024))
def test_horizon_implies_a_complete_window_and_a_whole_row(n_fft):
    S, cp = n_fft + n_fft // 4, n_fft // 4
    for reps in (1, 2, 3):
        W = reps * S
        for D in (1, 2, 24, 56):
            H = T.horizon(S, reps, D)
            for b in sorted({0, 1, 4, cp - 1, cp}):
                for d1 in (0, 1, S + b - 1, S + b, S + b + 1, 7 * S + 3, 100_001):
                    for Tn in (d1 + H, d1 + H + 1, d1 + H + 2 * S + 1):
                        valid = Tn - W - S + 1
                        assert d1 + W <= valid - 1                              # the peak window [d1, d1 + W] is complete
                        for d_hat in (d1, d1 + 1, d1 + W - 1, d1 + W):
                            g = P.geometry(Tn, S, b, d_hat, D)
                            Rw = P.row_samples(Tn, S, D)
                            assert Rw == (10 + D) * S + 2 and g.r + Rw <= Tn and g.row_len == Rw   # the whole row lies inside the stream
                            # ... so the row's fields do not move when the stream grows
                            for later in (Tn + 1, Tn + 12345):
                                g2 = P.geometry(later, S, b, d_hat, D)
                                assert (g2.r, g2.d_rel, g2.row_len) == (g.r, g.d_rel, g.row_len)
                                assert P.prepare(g2.row_len, g2.d_rel, S, b, D, 24) == P.prepare(g.row_len, g.d_rel, S, b, D, 24)
                    # ... and H is the least such bound up to the row's slack of L + b + 1: with fewer than H - L - b - 1 samples behind d1
                    # the latest peak's row is cut
                    short = d1 + H - (S + b + 1) - 1
                    g = P.geometry(short, S, b, d1 + W, D)
                    assert g.r + (10 + D) * S + 2 > short


# ---------------------------------------------------------------------------------------------------------- 2: the retention
def test_retention_bound_and_later_row_starts():
    for n_fft in (64, 256, 1024):
        S, cp = n_fft + n_fft // 4, n_fft // 4
        for reps in (1, 2, 3):
            W = reps * S
            for D in (1, 24, 56):
                H = T.horizon(S, reps, D)
                for b in (0, 4, cp):
                    for Tn in (1, W + S - 1, W + S, H - 1, H, H + 1, 3 * H + 7, 3 * H + 8):
                        valid = Tn - W - S + 1
                        los = set()
                        for d1 in range(max(Tn - H + 1, 0), max(valid, 0), max(H // 7, 1)):   # a deferred detection: d1 < valid, d1 + H > T
                            los.add(d1)
                        los |= {max(valid, 0), max(valid, 0) + 1, Tn, Tn + 5 * S}                # nothing deferred: lo >= valid
                        for lo in los:
                            for B in {0, max(min(lo - S - b, Tn), 0) & ~1}:
                                if B > max(lo - S - b, 0):
                                    continue
                                k = T.retained_from(lo, S, b, B, Tn)
                                assert k % 2 == 0 and B <= k <= Tn
                                assert Tn - k <= H + S + b + 2                       # so a window never exceeds this + max_chunk
                                for d_hat in (lo, lo + 1, lo + W):                   # every later detection: d_hat >= d1 >= lo
                                    assert (max(d_hat - S - b, 0) & ~1) >= k, (lo, B, Tn, d_hat, k)
    assert T.window_bound(80, 3, 24, 4, 4096) == T.horizon(80, 3, 24) + 80 + 4 + 2 + 4096


# ---------------------------------------------------------------------------------------------------------- 3: the model is the definition
def _key(p):
    return (p["d1"], p["d_hat"], np.float64(p["scan_f_delta"]).view(np.int64).item(), np.float32(p["metric"]).view(np.int32).item(),
            p["status"], p["offset"], p["len"], p["bytes"], np.float64(p["f_delta"]).view(np.int64).item())


@pytest.mark.parametrize("name", ("n64_a", "n256"))
def test_window_reproduces_the_deliveries(orc, name):
    b = P.built(orc, name)
    D = P.CASES[name]
    holdoff = min(b.frame_samples) - b.W
    assert R.certified(b.x, b.L, b.W, R.THRESHOLD, b.sums)
    w = T.whole(orc, b.x, b.n_fft, R.REPS, R.THRESHOLD, holdoff, True, 4, D, sums=b.sums)
    n, nd = len(b.x), len(w.scan.d1)
    assert nd == len(b.frame_samples)
    want_all = []
    for k, p in enumerate(w.packets):
        q = dict(p, d1=w.scan.d1[k], d_hat=w.scan.d_hat[k], scan_f_delta=w.scan.f_delta[k])
        want_all.append(_key(q))
    mid = nd // 2
    parts = {"one": [n], "4096": T.cuts_equal(n, 4096), "997": T.cuts_equal(n, 997),
             "edges": T.cuts_edges(n, w.scan.d1[mid], w.scan.d_hat[mid], w.H, b.S, 4)}
    bound = 0
    for what, sizes in parts.items():
        _, per_push = T.deliveries(orc, b.x, sizes, b.n_fft, R.REPS, R.THRESHOLD, holdoff, True, 4, D, w=w)
        assert sorted(k for ks in per_push for k in ks) == list(range(nd))                   # each packet exactly once
        for cap in ((256, 2) if what == "997" else (256,)):
            win = T.Window(orc, b.n_fft, R.REPS, R.THRESHOLD, holdoff, True, 4, D, scan_cap=cap)
            at = 0
            for i, m in enumerate(sizes):
                got = win.push(b.x[at: at + m], flush=i == len(sizes) - 1)
                at += m
                assert [_key(p) for p in got] == [want_all[k] for k in per_push[i]], (name, what, cap, i)
                assert win.keep_from % 2 == 0 and win.keep_from <= min(win.lo, win.T)
            bound = max(bound, win.max_window - max(sizes))
            assert win.max_window <= T.window_bound(b.S, R.REPS, D, 4, max(sizes)), (name, what)
    # a push of the whole capture walked in pieces of 4096 inside: everything arrives with it
    win = T.Window(orc, b.n_fft, R.REPS, R.THRESHOLD, holdoff, True, 4, D, max_chunk=4096)
    assert [_key(p) for p in win.push(b.x, flush=True)] == want_all
    assert win.max_window <= T.window_bound(b.S, R.REPS, D, 4, 4096)
    # the edge cuts do what they are for: the push that ends one sample short of the horizon does not deliver the packet, the next does
    _, per_push = T.deliveries(orc, b.x, parts["edges"], b.n_fft, R.REPS, R.THRESHOLD, holdoff, True, 4, D, w=w)
    ends = T.ends_of(parts["edges"])
    i = ends.index(w.scan.d1[mid] + w.H)
    assert mid in per_push[i] and ends[i - 1] == w.scan.d1[mid] + w.H - 1 and mid not in per_push[i - 1]


def test_share_rule():
    assert T.share([0, 10, 50], 5, [4, 5, 20, 54, 60]) == [[], [0], [1], [], [2]]
    assert T.share([0, 10, 50], 5, [4, 20], flush=True) == [[], [0, 1, 2]]
    assert T.share([0, 10, 50], 5, [4, 20], flush=False) == [[], [0, 1]]
    assert T.cuts_at(100, 0, 10, 10, 99, 100, 140) == [10, 89, 1] and sum(T.cuts_random(12345, 3)) == 12345


# ---------------------------------------------------------------------------------------------------------- 4: the surface
def test_surface_in_every_layer():
    import ofdm_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofdm_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    api = open(os.path.join(ROOT, "ofdm_amd", "api.py")).read()
    for f in NEW:
        assert re.search(r"\bint %s\(" % f, hdr), f
        assert f in ofdm_amd.SIGNATURES, f
        assert re.search(r"pub fn %s\s*\(" % f, rs), f
        assert f in hpp, f
        assert f in api or f == "ofdm_stream_destroy" and "ofdm_stream_destroy" in api, f
        # the handle comes first (ofdm_stream_create: its address): none of them is an `ofdm_ctx *ctx` entry point
        assert re.search(r"\b%s\(\s*(const\s+)?ofdm_stream\s*\*" % f, hdr), f
    assert "typedef struct ofdm_stream ofdm_stream;" in hdr and "class Stream" in hpp and "struct Stream" in rs
    assert "kernels_stream.hip" in open(os.path.join(ROOT, "ofdm_amd", "build.py")).read()


# ---------------------------------------------------------------------------------------------------------- 5: NULL handles
def test_null_handles_are_invalid_without_a_gpu():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    import ofdm_amd

    for f in NEW:
        fn = getattr(lib, f)
        fn.restype, fn.argtypes = ofdm_amd.SIGNATURES[f]
    INVALID = -1
    h, n, more = C.c_void_p(), C.c_int64(7), C.c_int32(7)
    assert lib.ofdm_stream_create(None, None, 8, 1, 4096, 0) == INVALID
    assert lib.ofdm_stream_create(C.byref(h), None, 8, 1, 4096, 0) == INVALID and not h.value
    assert lib.ofdm_stream_destroy(None) == INVALID and lib.ofdm_stream_reset(None, 0) == INVALID
    x = np.zeros(16, np.complex64)
    assert lib.ofdm_stream_push(None, x.ctypes.data, 16, 0, 0, None, 0, None, None, None, None, None, None, None, C.byref(n), C.byref(more)) == INVALID
    assert lib.ofdm_stream_push_sc16(None, x.ctypes.data, 16, 1.0, 0, 0, None, 0, None, None, None, None, None, None, None, C.byref(n),
                                     C.byref(more)) == INVALID
    assert lib.ofdm_stream_state(None, None, None, None, None) == INVALID
