"""GPU checks of ofdm_sc_scan_long (EXT-12: k_sc_mark + k_sc_walk + k_sc_peaks) against tests/scan_ref.py -- the holdoff rule in numpy f64
with the peaks from orc.sc_sync(capture[lo_k:]) -- on the certified captures of scan_ref.CAPTURES (tests/test_scan_cpu.py certifies
them): two N = 64 captures of about 40 000 samples and one N = 256 capture of 60 000, each 5 - 7 frames of two lengths at 15 dB with CFO,
a frame at sample 0, a gap shorter than W, and a last frame cut by the capture's end.

Required: d1 and d_hat equal the reference exactly, |f_delta - ref| <= 1e-9, |metric - ref| <= 1e-6 (the bars tests/test_gpu_host_path.py
holds ofdm_sc_correlate_long to), n_det and `more` equal, and for every k ofdm_sc_correlate_long(lag_lo = lo_k, lag_hi) returns the same
detection (d_hat equal; f_delta and metric inside the same two bars: the slice search sums by prefix differences, the scan in order).

The reference is computed once per (capture, holdoff, lag range) with no detection limit; a limit max_det keeps its first max_det
detections and sets more = (max_det < count), which is the rule (tests/test_scan_cpu.py holds scan_ref to the oracle loop for it).
At N = 256 the holdoff = 1 case runs over the lags [0, 700), one plateau and 577 detections: the reference takes the oracle's peak
search per detection, and the 8 024 crossings of the whole capture would cost it 17 s on the CPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import sc_margin_cases as smc
import scan_ref as R
from util import through_channel, wide

pytestmark = pytest.mark.gpu

DISPATCH = "k_sc_mark+k_sc_walk+k_sc_peaks"
ALL = 10 ** 6


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


@functools.lru_cache(maxsize=None)
def reference(orc, name, holdoff, lag_lo=0, lag_hi=0):
    b = R.build_capture(orc, name)
    return R.scan(orc, b.x, b.L, R.REPS, R.THRESHOLD, holdoff, ALL, lag_lo, lag_hi, b.sums)


def limited(ref, max_det):
    k = min(max_det, len(ref.d1))
    return R.Scan(ref.lo[:k], ref.d1[:k], ref.d_hat[:k], ref.f_delta[:k], ref.metric[:k], max_det < len(ref.d1))


def same_as_reference(got, want, what):
    assert got["d1"].tolist() == list(want.d1), (what, got["d1"][:8], want.d1[:8])
    assert got["d_hat"].tolist() == list(want.d_hat), what
    assert got["lag_lo"].tolist() == list(want.lo), what
    assert got["more"] == want.more, what
    if want.d1:
        fd_err = float(np.max(np.abs(got["f_delta"] - np.array(want.f_delta))))
        m_err = float(np.max(np.abs(got["metric"].astype(np.float64) - np.array(want.metric))))
        assert fd_err <= 1e-9 and m_err <= 1e-6, (what, fd_err, m_err)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("d1", "d_hat", "f_delta", "metric", "lag_lo")) and a["more"] == b["more"] \
        and a["next_lag_lo"] == b["next_lag_lo"]


def make_ctx(api, b, **kw):
    return api.Context(n_fft=b.n_fft, modulation=api.QAM16, guard_bands=True, sync_threshold=R.THRESHOLD, **kw)


def holdoff_cases(b):
    """(holdoff, lag_hi): 1, W, shortest frame - W, longer than the capture"""
    return ((1, 700 if b.n_fft == 256 else 0), (b.W, 0), (min(b.frame_samples) - b.W, 0), (len(b.x) + 5, 0))


@pytest.mark.parametrize("name", sorted(R.CAPTURES))
def test_scan_holdoffs_and_limits(api, orc, name):
    b = R.build_capture(orc, name)
    ctx = make_ctx(api, b)
    x = ctx.to_device(b.x)
    for holdoff, lag_hi in holdoff_cases(b):
        ref = reference(orc, name, holdoff, 0, lag_hi)
        count = len(ref.d1)
        assert count >= 1
        for max_det in (0, 1, count, count + 3):
            got = ctx.sc_scan_long(x, holdoff, max_det, 0, lag_hi)
            assert ctx.last_dispatch() == DISPATCH
            same_as_reference(got, limited(ref, max_det), (name, holdoff, max_det))
            assert got["more"] == (max_det < count)
        full = ctx.sc_scan_long(x, holdoff, count, 0, lag_hi)
        for k in range(count):                      # the existing long search from where detection k's search started
            d, fd, m = ctx.sc_correlate_long(x, int(full["lag_lo"][k]), lag_hi)
            assert d == full["d_hat"][k] and abs(fd - full["f_delta"][k]) <= 1e-9 and abs(m - float(full["metric"][k])) <= 1e-6, (name, holdoff, k)
    counts = [len(reference(orc, name, h, 0, hi).d1) for h, hi in holdoff_cases(b)]
    assert counts[0] > 500 and counts[1] == 2 * len(b.frame_samples) and counts[2] == len(b.frame_samples) and counts[3] == 1, counts


@pytest.mark.parametrize("name", sorted(R.CAPTURES))
def test_scan_lag_ranges_and_word_edge(api, orc, name):
    b = R.build_capture(orc, name)
    ctx = make_ctx(api, b)
    x = ctx.to_device(b.x)
    holdoff = min(b.frame_samples) - b.W
    whole = reference(orc, name, holdoff)
    starts = [st for st, _ in R.CAPTURES[name].frames]
    k = R.WORD_EDGE[name]
    ranges = [(whole.d1[0] + 20, 0),                          # lag_lo inside the first plateau
              (starts[2] - 100, whole.d1[4] + 30),            # both ends cut the capture; lag_hi inside a plateau: the peak window passes it
              (starts[1] + 5, whole.d1[3]),                   # lag_hi = a first crossing itself: that detection is outside
              (whole.d1[k] - 63, 0),                          # detection k on bit 63 of a bitmap word, k + 1 on bit 0 of a later one
              (whole.d1[-1] + 1, 0), (len(b.x), 0)]           # from the last plateau on; from behind the last lag
    for lag_lo, lag_hi in ranges:
        for h in (holdoff, 1) if (lag_lo, lag_hi) == ranges[2] and b.n_fft == 64 else (holdoff,):
            ref = reference(orc, name, h, lag_lo, lag_hi)
            got = ctx.sc_scan_long(x, h, ALL, lag_lo, lag_hi)
            same_as_reference(got, ref, (name, h, lag_lo, lag_hi))
            assert not got["more"]
    edge = ctx.sc_scan_long(x, holdoff, ALL, whole.d1[k] - 63, 0)
    assert (edge["d1"][0] - (whole.d1[k] - 63)) % 64 == 63 and (edge["d1"][1] - (whole.d1[k] - 63)) % 64 == 0
    cut = ctx.sc_scan_long(x, holdoff, ALL, starts[2] - 100, whole.d1[4] + 30)
    assert cut["d1"].tolist() == whole.d1[2:5] and cut["d_hat"][-1] > whole.d1[4] + 30
    assert ctx.sc_scan_long(x, holdoff, ALL, starts[1] + 5, whole.d1[3])["d1"].tolist() == whole.d1[1:3]


def test_scan_without_a_detection(api, orc):
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    for n in (40_000, 321, 320, 319, 100, 0):         # noise only; two lags, one lag, no lag (shorter than W + L), nothing at all
        noise = R.noise_capture(n)
        assert R.scan(orc, noise, 80, 3, 0.5, 1, 5).d1 == []
        x = ctx.to_device(noise) if n else ctx.empty((0,), __import__("torch").complex64)
        got = ctx.sc_scan_long(x, 1, 5)
        assert got["d1"].size == 0 and got["d_hat"].size == 0 and not got["more"] and got["next_lag_lo"] == 0, n
        assert ctx.last_dispatch() == (DISPATCH if n >= 320 else ""), (n, ctx.last_dispatch())
        got = ctx.sc_scan_long_host(noise, 1, 5)
        assert got["d_hat"].size == 0 and not got["more"], n


def test_scan_is_the_same_for_every_grid(api, orc):
    for name in ("n64_a", "n256"):
        b = R.build_capture(orc, name)
        x = None
        for holdoff, lag_hi in holdoff_cases(b)[:3]:
            runs = []
            for cap in (0, 1, 3):
                ctx = make_ctx(api, b, tuning={"grid_cap": cap})
                x = ctx.to_device(b.x) if x is None else x
                runs.append(ctx.sc_scan_long(x, holdoff, ALL, 0, lag_hi))
                assert ctx.last_dispatch() == DISPATCH
            assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), (name, holdoff)
            same_as_reference(runs[1], reference(orc, name, holdoff, 0, lag_hi), (name, holdoff, "grid_cap 1"))


def test_scan_host_form_and_mark_only(api, orc):
    b = R.build_capture(orc, "n64_b")
    ctx = make_ctx(api, b)
    holdoff = min(b.frame_samples) - b.W
    dev = ctx.sc_scan_long(ctx.to_device(b.x), holdoff, ALL, 11, 0)
    same_as_reference(dev, reference(orc, "n64_b", holdoff, 11, 0), "device form")
    assert same_bits(dev, ctx.sc_scan_long_host(b.x, holdoff, ALL, 11, 0))              # pageable
    assert ctx.last_dispatch() == DISPATCH
    pin = api.pinned_empty((len(b.x),), np.complex64)
    pin[:] = b.x
    assert ctx.lib.ofdm_host_is_pinned(pin.ctypes.data, pin.nbytes) == 1
    assert same_bits(dev, ctx.sc_scan_long_host(pin, holdoff, ALL, 11, 0))
    # optional outputs: d_hat and n_det alone
    dh, nd = np.zeros(16, np.int64), C.c_int64()
    x = ctx.to_device(b.x)
    assert ctx.lib.ofdm_sc_scan_long(ctx.h, C.c_void_p(x.data_ptr()), x.numel(), 11, 0, holdoff, 16, None, C.c_void_p(dh.ctypes.data), None, None,
                                     C.byref(nd), None) == 0
    assert nd.value == dev["d_hat"].size and dh[: nd.value].tolist() == dev["d_hat"].tolist() and not dh[nd.value:].any()
    # the laboratory key: k_sc_mark alone, nothing reported
    ctx.set_tuning("scan_mark_only", 1)
    got = ctx.sc_scan_long(x, holdoff, ALL)
    assert ctx.last_dispatch() == "k_sc_mark" and got["d_hat"].size == 0 and not got["more"]
    ctx.set_tuning("scan_mark_only", 0)
    assert same_bits(dev, ctx.sc_scan_long(x, holdoff, ALL, 11, 0))


def test_scan_error_codes(api):
    INVALID, UNSUPPORTED = -1, -2
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    x = ctx.to_device(R.noise_capture(1000))
    xp, n = C.c_void_p(x.data_ptr()), x.numel()
    dh, nd, more = np.zeros(4, np.int64), C.c_int64(7), C.c_int32(7)
    dhp = C.c_void_p(dh.ctypes.data)
    for scan, src in ((ctx.lib.ofdm_sc_scan_long, xp), (ctx.lib.ofdm_sc_scan_long_host, C.c_void_p(R.noise_capture(1000).ctypes.data))):
        call = lambda n=n, lo=0, hi=0, holdoff=1, max_det=4, src=src, dh=dhp, ndp=C.byref(nd): scan(ctx.h, src, n, lo, hi, holdoff, max_det, None, dh,
                                                                                                     None, None, ndp, C.byref(more))
        assert call() == 0 and nd.value == 0 and more.value == 0
        assert call(holdoff=0) == INVALID and call(holdoff=-3) == INVALID and call(max_det=-1) == INVALID
        assert call(src=None) == INVALID and call(dh=None) == INVALID and call(ndp=None) == INVALID
        assert call(n=-1) == INVALID and call(lo=-1) == INVALID
        assert call(n=0, src=None) == 0                                  # nothing to read: no pointer needed
        assert call(n=2 ** 40 + 1) == UNSUPPORTED                        # checked before anything is read
    ref = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True, sync_mode=api.SYNC_REFERENCE)
    assert ref.lib.ofdm_sc_scan_long(ref.h, xp, n, 0, 0, 1, 4, None, dhp, None, None, C.byref(nd), None) == UNSUPPORTED
    with pytest.raises(api.OfdmError):
        ctx.sc_scan_long(x, 0, 4)


@pytest.mark.parametrize("n,late", smc.SIZES, ids=[f"N{n}{'late' if late else ''}" for n, late in smc.SIZES])
def test_scan_razor_margins(api, orc, n, late):
    """The razor-margin captures of tests/sc_margin_cases.py as one-detection scans: the threshold within 1e-6, 1e-9 and 1e-12 of a lag's
    own metric, on an ordinary capture and behind bursts that leave the windows 2^-9 .. 2^-17 of the capture's energy.  The scan that ends
    at the razor lag (lag_hi = d_k + 1) answers the decision itself: one detection with d1 = d_k, or none.  The scan over the case's
    n_lags must find the first crossing the oracle's metric shows (the razor lag decided by the certified verdict) and, where the case's
    bounded search saw the whole peak window, the oracle's d_hat, CFO and metric.  Every kept case of every family is asserted: the scan
    sums each window in the oracle's order, so no family is excused."""
    sz = smc.build(orc, n, late)
    ctx = api.Context(n_fft=n, modulation=api.QAM16, guard_bands=True)
    xs = [ctx.to_device(c) for c in sz.caps]
    compared = whole_window = 0
    for t in sz.thresholds:
        ctx.set_tuning("sync_threshold_bits", int(np.float64(t.thr).view(np.int64)))
        for ci, (row, razor) in enumerate(zip(t.rows, t.razor)):
            if row is None or razor is None:
                continue
            what = (n, late, smc.CAPTURES[ci], t.d, t.eps, t.sign)
            got = ctx.sc_scan_long(xs[ci], 1, 1, 0, t.d + 1)
            assert got["d1"].tolist() == ([t.d] if razor[0] >= 0 else []), (what, got["d1"], razor[0])
            assert razor[0] in (t.d, -1)
            ge = sz.metric[ci][: t.n_lags] >= t.thr
            ge[t.d] = razor[0] >= 0
            want_d1 = int(np.nonzero(ge)[0][0]) if ge.any() else -1
            got = ctx.sc_scan_long(xs[ci], sz.W + 1, 1, 0, t.n_lags)
            assert ctx.last_dispatch() == DISPATCH
            assert got["d1"].tolist() == ([want_d1] if want_d1 >= 0 else []), (what, got["d1"], want_d1)
            assert (want_d1 >= 0) == (row[0] >= 0), what
            compared += 1
            if want_d1 >= 0 and want_d1 + sz.W <= t.n_lags - 1:
                wd, _, wm, wfd = row
                assert got["d_hat"][0] == wd and abs(got["f_delta"][0] - wfd) <= 1e-9 and abs(got["metric"][0] - wm) <= 1e-6 * max(1.0, wm), what
                whole_window += 1
    kept = sum(c.kept for c in sz.cases)
    print(f"N = {n}{' late' if late else ''}: {compared} rows compared ({kept} kept cases), {whole_window} with the whole peak window")
    assert compared >= kept > 0 and whole_window >= 0.9 * compared


def test_decode_all_returns_what_was_sent(api, orc):
    """api.decode_all on a capture of six framed, frame-checked packets of two sizes (QPSK, rate 1/2, 25 dB): with the real frame size as
    holdoff exactly the packets sent come back, in order, each equal to decode_long from where its search started; with the default
    holdoff (the shortest frame) every further detection inside a payload is reported with a failed status, never as a packet."""
    rng = np.random.default_rng(2024)
    ecc = api.ECC_CONV_K7F_R12
    sizes = (60, 150, 60, 150, 150, 60)
    ctx = api.Context(n_fft=64, modulation=api.QPSK, guard_bands=True, ecc=ecc + api.ECC_FCS)
    pays = [bytes(rng.integers(0, 256, s, dtype=np.uint8)) for s in sizes]
    frames = [api.encode(p, True, api.QPSK, 64, ecc=ecc, fcs=True) for p in pays]
    span, at, cap = 0, [], []
    for f in frames:
        at.append(span + int(rng.integers(100, 900)))
        span = at[-1] + f.size + 64
    cap = np.zeros(span + 700, np.complex128)
    for st, f in zip(at, frames):
        seg = wide(through_channel(orc, rng, f, f.size + 64, 0, (rng.random() * 1.8 - 0.9) * np.pi / 80, snr_db=None, data_start=800))
        cap[st: st + seg.size] += seg
    sigma = np.sqrt(float(np.mean(np.abs(frames[0][800:]) ** 2)) / 10 ** 2.5 / 2)
    cap = (cap + sigma * (rng.standard_normal(cap.size) + 1j * rng.standard_normal(cap.size))).astype(np.complex64)
    W = 240
    D = max((f.size + 79) // 80 for f in frames) - 10
    holdoff = min(f.size for f in frames) - W
    kw = dict(guard_bands=True, modulation=api.QPSK, n_fft=64, ecc=ecc, fcs=True, max_symbols=D)
    got = api.decode_all(cap, holdoff=holdoff, **kw)
    assert [g["status"] for g in got] == [api.FRAME_OK] * len(pays) and [g["bytes"] for g in got] == pays
    assert all(0 <= g["offset"] - st < 80 for g, st in zip(got, at)) and not any(g["more"] for g in got)
    x = ctx.to_device(cap)
    det = ctx.sc_scan_long(x, holdoff, 4096)
    for k, g in enumerate(got):                       # the loop it stands for
        one = ctx.decode_long(x, D, lag_lo=int(det["lag_lo"][k]))
        assert (one["status"], one["len"], one["offset"], one["f_delta"], one["metric"]) == (g["status"], g["len"], g["offset"], g["f_delta"], g["metric"])
        assert g["d_hat"] == det["d_hat"][k] and g["d1"] == det["d1"][k]
    loose = api.decode_all(cap, **kw)                 # holdoff=None: 11 S - W
    assert [g["bytes"] for g in loose if g["status"] == api.FRAME_OK] == pays
    assert all(g["status"] in (api.FRAME_OK, api.FRAME_HEADER, api.FRAME_FCS, api.FRAME_SHORT) for g in loose)
    two = api.decode_all(cap, holdoff=holdoff, max_packets=2, **kw)
    assert [g["bytes"] for g in two] == pays[:2] and [g["more"] for g in two] == [False, True]
