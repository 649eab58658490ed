"""GPU checks of the streaming receiver (EXT-14: ofdm_stream_create / _push / _push_sc16 / _reset / _state; k_stream_ingest<fc32> and
k_stream_ingest<sc16> in front of the scan's and the decode's kernels).

The contract (include/ofdm_hip.h, "a streaming receiver"): however the stream is cut into pushes, the packets delivered are, field for
field and bit for bit, those of ONE ofdm_rx_decode_all_long_host call on the concatenation, each exactly once, and packet k arrives with
the first push after which T >= d1_k + H (or with the flush) and with no other.  Every case on the captures of scan_ref.CAPTURES compares
two ways:
  (a) bit for bit, every field and the push that delivered it, against Context.decode_all_host of the whole capture on a SECOND context
      (existing code, not code under test);
  (b) against stream_ref.deliveries (the whole-stream scan of scan_ref plus packets_ref on the whole capture, shared out by the horizon
      rule) by the bars of tests/test_gpu_scan.py and tests/test_gpu_packets.py: d1, d_hat, status, offset, out_len exact, bytes through
      util.assert_bytes_match, |f_delta - ref| <= 1e-9, |metric - ref| <= 1e-6.
The mode families (captures from tools/link.py, as tests/test_gpu_packets.py builds its own) have no numpy restatement of their decoders
in packets_ref: they are held to (a), to the delivery rule with the reference call's d1, and to the payloads that were sent.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import packets_ref as P
import scan_ref as R
import sc16_ref
import stream_ref as T
from util import assert_bytes_match

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.link import data_snr, link_on, wide_link_on  # noqa: E402

pytestmark = pytest.mark.gpu

MOD = 4
NAMES = ("n64_a", "n64_b", "n256")
INGEST = ("k_stream_ingest<fc32>", "k_stream_ingest<sc16>")
SCAN = "k_sc_mark+k_sc_walk+k_sc_peaks"


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def bits64(v):
    return np.float64(v).view(np.int64).item()


def bits32(v):
    return np.float32(v).view(np.int32).item()


def key(r, k):
    """everything delivered for packet k of a result dict, floats as their bit patterns"""
    n = int(r["len"][k]) if int(r["status"][k]) == 0 else 0
    return (int(r["d1"][k]), int(r["d_hat"][k]), int(r["status"][k]), int(r["len"][k]), int(r["offset"][k]), bits64(r["f_delta"][k]),
            bits32(r["metric"][k]), bytes(r["bytes"][k, :max(n, 0)]))


def keys(r):
    return [key(r, k) for k in range(len(r["status"]))]


def run(s, x, sizes, flush=True, sc16_scale=None, max_pkt=64):
    """push x in pieces of `sizes`, the last with flush -> per push the keys it delivered"""
    out, at = [], 0
    for i, m in enumerate(sizes):
        out.append(keys(s.push_all(x[at: at + m], flush and i == len(sizes) - 1, sc16_scale=sc16_scale, max_pkt=max_pkt)))
        at += m
    assert at == len(x)
    return out


# ---------------------------------------------------------------------------------------------------------- the captures and their answers
class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(api, orc, name, small_holdoff=False):
    c = Case()
    c.b = P.built(orc, name)
    c.D = P.CASES[name]
    c.holdoff = c.b.S if small_holdoff else min(c.b.frame_samples) - c.b.W
    kw = dict(n_fft=c.b.n_fft, modulation=api.QAM16, guard_bands=True, sync_threshold=R.THRESHOLD)
    c.ctx, c.other = api.Context(**kw), api.Context(**kw)
    c.ref = c.other.decode_all_host(c.b.x, c.holdoff, 2048, c.D)                    # (a): the one-shot call, on the second context
    assert not c.ref["more"]
    c.want = keys(c.ref)
    c.H = T.horizon(c.b.S, R.REPS, c.D)
    c.w = T.whole(orc, c.b.x, c.b.n_fft, R.REPS, R.THRESHOLD, c.holdoff, True, MOD, c.D, sums=c.b.sums)   # (b): the definition
    assert len(c.w.scan.d1) == len(c.want) and c.w.H == c.H
    assert small_holdoff or len(c.want) == len(c.b.frame_samples)
    return c


def check_b(c, got, first=0):
    """(b): every delivered packet against the definition"""
    for g in got:
        k = c.w.scan.d1.index(g[0] - first)
        w, what = c.w.packets[k], (c.b.name, k)
        assert g[1] - first == c.w.scan.d_hat[k] and (g[2], g[3]) == (w["status"], w["len"]) and g[4] - first == w["offset"], (what, g[:5], w["status"], w["offset"])
        fd, m = np.int64(g[5]).view(np.float64), np.int32(g[6]).view(np.float32)
        assert abs(float(fd) - w["f_delta"]) <= 1e-9 and abs(float(m) - float(c.w.scan.metric[k])) <= 1e-6, (what, fd, m)
        if w["status"] == 0:
            assert_bytes_match(g[7], w["bytes"], w["soft"][128 // MOD:], MOD, what=str(what))


def check(c, per_push, sizes, flush=True):
    """(a) with the push that delivered every packet, then (b)"""
    share = T.share([int(d) for d in c.ref["d1"]], c.H, T.ends_of(sizes), flush)
    for i, (got, ks) in enumerate(zip(per_push, share)):
        assert got == [c.want[k] for k in ks], (c.b.name, i, sizes[i], [g[:5] for g in got], ks)
    check_b(c, [g for got in per_push for g in got])
    return share


# ---------------------------------------------------------------------------------------------------------- partitions
def partitions(c):
    n, d1, dh = len(c.b.x), c.w.scan.d1, c.w.scan.d_hat
    parts = {"one": [n], "4096": T.cuts_equal(n, 4096), "997": T.cuts_equal(n, 997), "random": T.cuts_random(n, 1400 + c.b.n_fft)}
    for tag, k in (("first", 0), ("middle", len(d1) // 2), ("last", len(d1) - 1)):
        parts["edges_" + tag] = T.cuts_edges(n, d1[k], dh[k], c.H, c.b.S, 4)
    k = 1
    at = d1[k] + c.H - 150
    parts["single_samples"] = [at] + [1] * 300 + [n - at - 300]
    parts["empty_between"] = [m for size in T.cuts_equal(n, 4096) for m in (size, 0)] + [0]
    return parts


@pytest.mark.parametrize("name", NAMES)
def test_every_partition_is_the_one_shot_call(api, orc, name):
    c = case(api, orc, name)
    n = len(c.b.x)
    assert int(c.ref["d1"][0]) == 0 or int(c.ref["offset"][0]) < c.b.S                         # a frame at sample 0
    assert P.last_is_cut(c.b, c.w.packets[-1])                                                 # a last frame cut by the end
    with c.ctx.stream(c.D, c.holdoff, max_chunk=16384) as s:
        for what, sizes in partitions(c).items():
            s.reset()
            share = check(c, run(s, c.b.x, sizes), sizes)
            st = s.state()
            assert st["total"] == n and st["ended"] and st["kept_from"] % 2 == 0, (what, st)
            if what == "single_samples":                                                       # exactly the push that reaches the horizon
                i = T.ends_of(sizes).index(c.w.scan.d1[1] + c.H)
                assert 1 in share[i] and 1 not in [k for ks in share[:i] for k in ks]
    # one push of the whole capture walked in pieces of 4096 inside the call: everything arrives with it
    with c.ctx.stream(c.D, c.holdoff, max_chunk=4096) as s:
        check(c, run(s, c.b.x, [n]), [n])
        assert c.ctx.last_dispatch().startswith(INGEST[0] + "+" + SCAN)
    # max_pkt = 1, drained through `more`
    with c.ctx.stream(c.D, c.holdoff, max_chunk=16384) as s:
        sizes, per_push, at, mores = T.cuts_equal(n, 16384), [], 0, 0
        for i, m in enumerate(sizes):
            flush = i == len(sizes) - 1
            r = s.push(c.b.x[at: at + m], flush, max_pkt=1)
            got = keys(r)
            while r["more"]:
                mores += 1
                r = s.push(None, flush, max_pkt=1)
                assert len(r["status"]) == 1
                got += keys(r)
            per_push.append(got)
            at += m
        assert mores >= 2
        check(c, per_push, sizes)
    # the laboratory key: two detections per scan + decode round, so the round loop runs and resumes behind a round's last detection
    c.ctx.set_tuning("stream_scan_cap", 2)
    try:
        with c.ctx.stream(c.D, c.holdoff, max_chunk=65536) as s:
            for sizes in ([n], T.cuts_equal(n, 16384)):
                s.reset()
                check(c, run(s, c.b.x, sizes), sizes)
    finally:
        c.ctx.set_tuning("stream_scan_cap", 0)


def test_small_holdoff_delivers_the_crossings_inside_payloads(api, orc):
    c = case(api, orc, "n64_a", True)
    assert c.holdoff == c.b.S and len(c.want) > 3 * len(c.b.frame_samples)
    assert len({w[2] for w in c.want}) > 1                                                     # with their statuses
    with c.ctx.stream(c.D, c.holdoff, max_chunk=4096) as s:
        for sizes in (T.cuts_equal(len(c.b.x), 997), [len(c.b.x)]):
            s.reset()
            check(c, run(s, c.b.x, sizes, max_pkt=16), sizes)


# ---------------------------------------------------------------------------------------------------------- sc16
def test_sc16_pushes_are_the_pushes_of_the_widened_samples(api, orc):
    c = case(api, orc, "n64_a")
    q, scale = sc16_ref.quantise(c.b.x, 0.9)
    xw = sc16_ref.widen(q, scale)
    assert np.array_equal(xw, api.sc16_widen(q, scale))
    sizes = T.cuts_equal(len(xw), 997)
    ref = c.other.decode_all_host(xw, c.holdoff, 64, c.D)
    with c.ctx.stream(c.D, c.holdoff, max_chunk=4096) as s16, c.ctx.stream(c.D, c.holdoff, max_chunk=4096) as s32:
        got16, disp, at = [], [], 0
        for i, m in enumerate(sizes):
            got16.append(keys(s16.push_all(q[at: at + m], i == len(sizes) - 1, sc16_scale=scale)))
            disp.append(c.ctx.last_dispatch())
            at += m
        got32 = run(s32, xw, sizes)
    assert got16 == got32
    assert [g for got in got16 for g in got] == keys(ref) and len(ref["status"]) == len(c.b.frame_samples)
    share = T.share([int(d) for d in ref["d1"]], c.H, T.ends_of(sizes))
    assert [len(g) for g in got16] == [len(ks) for ks in share]
    assert all(d.startswith("k_stream_ingest<sc16>") for d in disp), disp
    # (b): the definition on the widened capture
    assert R.certified(xw, c.b.L, c.b.W, R.THRESHOLD)
    w = T.whole(orc, xw, c.b.n_fft, R.REPS, R.THRESHOLD, c.holdoff, True, MOD, c.D)
    cw = Case()
    cw.b, cw.w = c.b, w
    check_b(cw, [g for got in got16 for g in got])
    with c.ctx.stream(c.D, c.holdoff) as s:                                                    # a bad scale
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(api.OfdmError):
                s.push(q[:100], sc16_scale=bad)
        with pytest.raises(api.OfdmError):
            s.push(q[:100])


# ---------------------------------------------------------------------------------------------------------- mode families
GAPS = (0, 37, 402, 3, 1211, 90, 15, 700)


def _families(api):
    coded = dict(n=64, mod=api.QPSK, frames=8, payload=120, snr=25.0, kw={}, wide=False)
    return {
        "conv_k7f_r12": dict(coded, ecc=api.ECC_CONV_K7F_R12),
        "ldpc648": dict(coded, ecc=api.ECC_LDPC648),
        "fcs_rs255_k7f_r34": dict(coded, ecc=api.ECC_FCS + api.ECC_RS255_K7F_R34),
        "hamming74_soft": dict(coded, ecc=api.ECC_HAMMING74_SOFT),
        "chest_wls": dict(coded, mod=api.QAM16, ecc=api.ECC_NONE, snr=30.0, kw=dict(chest_mode=api.CHEST_WLS)),
        "cfo_wide": dict(coded, ecc=api.ECC_CONV_K7F_R34, kw=dict(cfo_mode=api.CFO_WIDE), wide=True),
        "llrw_noise": dict(coded, ecc=api.ECC_LDPC648, kw=dict(llr_weight=api.LLRW_NOISE)),
        "n1024_hamming74": dict(coded, n=1024, ecc=api.ECC_HAMMING74, frames=3, payload=900, snr=float(data_snr(1024, 30.0))),
    }


FAMILIES = ("conv_k7f_r12", "ldpc648", "fcs_rs255_k7f_r34", "hamming74_soft", "chest_wls", "cfo_wide", "llrw_noise", "n1024_hamming74")


@pytest.mark.parametrize("fam", FAMILIES)
def test_mode_families_in_chunks_of_997(api, fam):
    f = _families(api)[fam]
    kw = dict(n_fft=f["n"], modulation=f["mod"], guard_bands=True, ecc=f["ecc"], **f["kw"])
    ctx, other = api.Context(**kw), api.Context(**kw)
    seed = 1400 + f["ecc"]
    pay, rx = (wide_link_on(ctx, f["frames"], f["payload"], f["snr"], seed)[:2] if f["wide"] else link_on(ctx, f["frames"], f["payload"], f["snr"], seed))
    rx, pay = rx.cpu().numpy(), pay.cpu().numpy()
    n_frames, span = rx.shape
    at, pos = [], 0
    for k in range(n_frames):                                  # the link's captures back to back with unequal gaps, 500 zeros behind the last
        pos += GAPS[k % len(GAPS)] * (ctx.S // 80)
        at.append(pos)
        pos += span
    x = np.zeros(pos + 500, np.complex64)
    for k, st in enumerate(at):
        x[st: st + span] = rx[k]
    D = ctx.data_symbols(f["payload"])
    holdoff = ctx.frame_samples(f["payload"]) - ctx.params.sync_window_reps * ctx.S
    ref = other.decode_all_host(x, holdoff, 64, D)
    want = keys(ref)
    assert len(want) == n_frames and all(w[2] == 0 and w[7][: f["payload"]] == bytes(pay[k]) for k, w in enumerate(want)), (fam, [w[:5] for w in want])
    sizes = T.cuts_equal(len(x), 997)
    with ctx.stream(D, holdoff, max_chunk=4096) as s:
        per_push = run(s, x, sizes)
        assert s.horizon == T.horizon(ctx.S, 3, D)
        share = T.share([int(d) for d in ref["d1"]], s.horizon, T.ends_of(sizes))
    for i, (got, ks) in enumerate(zip(per_push, share)):
        assert got == [want[k] for k in ks], (fam, i, [g[:5] for g in got], ks)


# ---------------------------------------------------------------------------------------------------------- first_sample, grid
def test_first_sample_beyond_2_to_the_33(api, orc):
    c = case(api, orc, "n64_b")
    first = 2 ** 33 + 7
    sizes = T.cuts_equal(len(c.b.x), 4096)
    with c.ctx.stream(c.D, c.holdoff, max_chunk=4096, first_sample=first) as s:
        got = run(s, c.b.x, sizes)
        assert s.state()["total"] == len(c.b.x)                # the state is stream-relative
        moved = [[(g[0] - first, g[1] - first) + g[2:4] + (g[4] - first,) + g[5:] for g in push] for push in got]
        check(c, moved, sizes)
        assert all(g[0] >= first and g[1] >= first and g[4] >= first for push in got for g in push)
        s.reset(3)                                             # ... and reset takes a new one
        again = run(s, c.b.x, sizes)
        assert [[(g[0] - 3, g[1] - 3) + g[2:4] + (g[4] - 3,) + g[5:] for g in push] for push in again] == moved


def test_grid_cap_changes_nothing(api, orc):
    c = case(api, orc, "n64_a")
    sizes = T.cuts_equal(len(c.b.x), 997)
    for cap in (1, 3):
        c.ctx.set_tuning("grid_cap", cap)
        try:
            with c.ctx.stream(c.D, c.holdoff, max_chunk=4096) as s:
                check(c, run(s, c.b.x, sizes), sizes)
        finally:
            c.ctx.set_tuning("grid_cap", 0)


# ---------------------------------------------------------------------------------------------------------- staleness
def test_nothing_depends_on_what_the_buffers_held(api, orc):
    a, b = case(api, orc, "n64_a"), case(api, orc, "n64_b")
    kw = dict(n_fft=64, modulation=api.QAM16, guard_bands=True, sync_threshold=R.THRESHOLD)
    # the rule of tests/test_gpu_ws_poison.py, honoured here: armed before create (the stream fills what it allocates), re-armed with other
    # bytes between pushes (the context's workspaces and host pipe are filled each time): the same answers
    ctx = api.Context(**kw)
    ctx.set_tuning("ws_poison", 0x1FF)
    sizes = T.cuts_equal(len(a.b.x), 4096)
    with ctx.stream(a.D, a.holdoff, max_chunk=4096) as s:
        per_push, at = [], 0
        for i, m in enumerate(sizes):
            ctx.set_tuning("ws_poison", 0x17F if i % 2 else 0x100)
            per_push.append(keys(s.push_all(a.b.x[at: at + m], i == len(sizes) - 1)))
            at += m
        check(a, per_push, sizes)
        # a stream that received capture X, was reset, then received Y equals a fresh stream on Y
        s.reset()
        sizes_b = T.cuts_equal(len(b.b.x), 997)
        check(b, run(s, b.b.x, sizes_b), sizes_b)
    ctx.set_tuning("ws_poison", 0)
    # two streams on one context with interleaved pushes each equal their own stream alone
    with ctx.stream(a.D, a.holdoff, max_chunk=4096) as sa, ctx.stream(b.D, b.holdoff, max_chunk=4096) as sb:
        sa_sizes, sb_sizes = T.cuts_equal(len(a.b.x), 4096), T.cuts_equal(len(b.b.x), 2500)
        ga, gb, ia, ib, pa, pb = [], [], 0, 0, 0, 0
        while ia < len(sa_sizes) or ib < len(sb_sizes):
            if ia < len(sa_sizes):
                ga.append(keys(sa.push_all(a.b.x[pa: pa + sa_sizes[ia]], ia == len(sa_sizes) - 1)))
                pa += sa_sizes[ia]
                ia += 1
            for _ in range(2):
                if ib < len(sb_sizes):
                    gb.append(keys(sb.push_all(b.b.x[pb: pb + sb_sizes[ib]], ib == len(sb_sizes) - 1)))
                    pb += sb_sizes[ib]
                    ib += 1
        check(a, ga, sa_sizes)
        check(b, gb, sb_sizes)


# ---------------------------------------------------------------------------------------------------------- dispatch
def test_dispatch_strings(api, orc):
    c = case(api, orc, "n64_a")
    d1 = c.w.scan.d1
    with c.ctx.stream(c.D, c.holdoff, max_chunk=16384) as s:
        r = s.push(c.b.x[:100])                                                  # a window without a valid lag: the ingest alone
        assert c.ctx.last_dispatch() == "k_stream_ingest<fc32>" and len(r["status"]) == 0
        r = s.push(c.b.x[100: d1[0] + c.H - 1])                                  # one sample short of the horizon: ingest + scan, nothing delivered
        assert c.ctx.last_dispatch() == "k_stream_ingest<fc32>+" + SCAN and len(r["status"]) == 0
        r = s.push(c.b.x[d1[0] + c.H - 1: d1[0] + c.H])                          # the sample that commits packet 0
        disp = c.ctx.last_dispatch()
        assert keys(r) == c.want[:1]
        assert disp.startswith("k_stream_ingest<fc32>+" + SCAN + "+k_pkt_rows+k_gather_rows+k_rx_prepare_rows") and disp.endswith("k_pkt_finish"), disp
        before = c.ctx.last_dispatch()
        r = s.push(None)                                                         # n = 0, no flush, nothing pending: a no-op
        assert len(r["status"]) == 0 and not r["more"] and c.ctx.last_dispatch() == before
        r = s.flush()                                                            # n = 0 with flush: no ingest
        assert c.ctx.last_dispatch().startswith(SCAN) or len(r["status"]) == 0


# ---------------------------------------------------------------------------------------------------------- errors
def test_error_codes(api, orc):
    INVALID, UNSUPPORTED = -1, -2
    c = case(api, orc, "n64_a")
    ctx, lib = c.ctx, c.ctx.lib
    h = C.c_void_p()
    mk = lambda ctx_h=ctx.h, D=c.D, holdoff=c.holdoff, chunk=4096, first=0: lib.ofdm_stream_create(C.byref(h), ctx_h, D, holdoff, chunk, first)
    assert mk(ctx_h=None) == INVALID and mk(D=0) == INVALID and mk(holdoff=0) == INVALID and mk(chunk=0) == INVALID and mk(first=-1) == INVALID
    assert lib.ofdm_stream_create(None, ctx.h, c.D, c.holdoff, 4096, 0) == INVALID and not h.value
    ref = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True, sync_mode=api.SYNC_REFERENCE)
    assert mk(ctx_h=ref.h) == UNSUPPORTED and not h.value
    assert mk() == 0 and h.value
    ob = ctx.decode_row_bytes(c.D)
    out, i32a, i32b = np.zeros((4, ob), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int32)
    i64a, i64b, i64c, f64, f32 = np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4), np.zeros(4, np.float32)
    nd, more = C.c_int64(7), C.c_int32(7)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    x = np.ascontiguousarray(c.b.x[:2500])                                      # fewer than the horizon: nothing commits without a flush
    q = sc16_ref.quantise(x, 0.9)[0]

    def push(x=x, n=2500, flush=0, max_pkt=4, out=out, stride=ob, ln=i32a, st=i32b, dh=i64c, fd=f64, m=f32, ndp=C.byref(nd), handle=h):
        return lib.ofdm_stream_push(handle, p(x), n, flush, max_pkt, p(out), stride, p(ln), p(st), p(i64a), p(fd), p(m), p(i64b), p(dh), ndp,
                                    C.byref(more))

    def push16(scale, handle=h):
        return lib.ofdm_stream_push_sc16(handle, p(q), 2500, scale, 0, 4, p(out), ob, p(i32a), p(i32b), p(i64a), p(f64), p(f32), p(i64b), p(i64c),
                                         C.byref(nd), C.byref(more))

    assert push(handle=None) == INVALID and push(n=-1) == INVALID and push(x=None) == INVALID and push(stride=ob - 1) == INVALID
    assert push(max_pkt=-1) == INVALID and push(ndp=None) == INVALID
    for name in ("out", "ln", "st", "dh", "fd", "m"):
        assert push(**{name: None}) == INVALID, name
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert push16(bad) == INVALID
    assert push16(1.0, handle=None) == INVALID
    t = C.c_int64(-1)
    assert lib.ofdm_stream_state(h, C.byref(t), None, None, None) == 0 and t.value == 0            # a refused push consumed nothing
    assert push() == 0 and nd.value == 0 and more.value == 0
    assert push(x=None, n=0, flush=1) == 0 and nd.value >= 1                                        # the flush: the frame at sample 0 and the next, cut at 2500
    assert more.value == 0
    assert push() == INVALID and push(x=None, n=0) == INVALID and push(x=None, n=0, flush=1) == INVALID     # ended
    assert lib.ofdm_stream_reset(h, -1) == INVALID and lib.ofdm_stream_reset(h, 0) == 0            # reset revives it
    assert push() == 0 and nd.value == 0
    assert lib.ofdm_stream_destroy(h) == 0
    with ctx.stream(c.D, c.holdoff, max_chunk=4096) as s:                                           # the same through the Python layer
        s.push(x, flush=True)
        with pytest.raises(api.OfdmError):
            s.push(x)
        s.reset()
        assert len(s.push(x)["status"]) == 0 and s.state()["total"] == 2500 and not s.state()["ended"]
    # a context that is closed takes its streams with it (a stream is destroyed before its context)
    tmp = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    s = tmp.stream(c.D, c.holdoff, max_chunk=4096)
    s.push(x)
    tmp.close()
    assert s.h is None
    s.close()
    got = list(api.receive_stream((c.b.x[i: i + 5000] for i in range(0, len(c.b.x), 5000)), c.D, True, api.QAM16, 64, holdoff=c.holdoff,
                                  sync_threshold=R.THRESHOLD))
    assert [(g["d1"], g["d_hat"], g["status"], g["offset"], g["bytes"]) for g in got] == [(w[0], w[1], w[2], w[4], w[7]) for w in c.want]
