"""The decode chain over the pairwise cover of its options (tests/cover_cases.py; DESIGN.md section 2, "The options meet"): every row
is a three-frame decode of the captures tests/test_cover_cpu.py picked, held to tests/receiver_ref.py --

  transmit      encode_batch against orc.encode of mode_encode, ||gpu - oracle|| / ||oracle|| <= 1e-5, lengths exact
  front end     status and offset exact, f_delta within 1e-9 rad/sample, the metric to f32 rounding (1e-6 max(1, M); the xcorr peak of
                SYNC_REFERENCE to 1e-5 of itself, the bar of its own tests)
  hard modes    the inner mode's bytes against the f64 oracle under util.assert_bytes_match (a decision is excused only where the
                oracle's point lies within 1e-5 of a boundary; Hamming: on the coded stream), the outer layers by the CPU rule, exact
  soft modes    status, len and bytes equal to the composition of the stage entry points, exact -- on the row's captures and on the
                same captures under heavy noise (cover_cases.stressed), where the decoders work at their edge and a wrong LLR shows
  dispatch      the trace names the kernels of the row's options (k_chest_solve, k_noise_bins, k_cfo_wide, k_xcorr) and no others
  entry points  chain_checks.assert_entry_points_agree; decode_host with the row's n_lags; the sc16 twins against the fc32 calls on
                the widened samples; under Schmidl-Cox the three captures laid end to end through sc_scan_long + decode_packets
  liveness      at least two of the three frames deliver the sent payload in the reference / composition, 90 % over the table

`pytest -m gpu tests/test_gpu_cover.py -s` prints every row's dispatch trace and, last, the kernel names the cover reached."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cover_cases as cc  # noqa: E402
import packets_ref as P  # noqa: E402
import receiver_ref as rr  # noqa: E402
import sc16_ref  # noqa: E402
from chain_checks import assert_entry_points_agree, assert_rows_are, assert_same_rows, ofdm_api as _api  # noqa: E402
from util import assert_bytes_match, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cc.cases()
LIVE = {}          # row -> frames of the three whose reference delivers the sent payload
DISPATCH = {}      # row -> the traces of its calls
EXCUSED = {}
STRESS = {}        # soft row -> (status, delivered) of its three frames under heavy noise


@functools.lru_cache(maxsize=None)
def _stage_context(n, mod, guard):
    """a context that knows none of a row's options: the stage entry points of receiver_ref.compose"""
    return _api().Context(n_fft=n, modulation=mod, guard_bands=guard)


def _host(r):
    return {key: v.cpu().numpy() for key, v in r.items()}


def _delivers(k, data, pay):
    """the reference row carries the sent payload (bare RS delivers whole blocks: the payload in front)"""
    return len(data) >= len(pay) and bytes(data[:len(pay)]) == bytes(pay) and (len(data) == len(pay) or k.outer == cc.OUTER_RS)


def _hard_rows(orc, k, s, inner_rows, captures, offsets, f_deltas, statuses, D):
    """the inner mode's delivered rows against the f64 oracle at the chain's own timing -> ({frame: (status, len, bytes)} of the whole
    mode by the CPU rule over the device's inner bytes, excused decisions)"""
    want, excused = {}, 0
    pad = bytes(16)
    for f, x32 in enumerate(captures):
        if statuses[f] != 0:
            want[f] = (int(statuses[f]), 0, b"")
            continue
        assert int(inner_rows["status"][f]) == 0, f
        got = bytes(inner_rows["bytes"][f, :int(inner_rows["len"][f])])
        body, soft = rr.hard_reference(orc, x32, k, int(offsets[f]), float(f_deltas[f]), D)
        if k.inner == 0:
            excused += assert_bytes_match(pad + got, pad + body, soft, k.mod, what=f"{k.id} frame {f}")
        elif got != rr.hard_finish(orc, 1, body):
            # the excuse is taken on the coded stream: the device's own hard bytes at the chain's timing
            hk = s.estimate_channel(captures_dev(s, x32), _i32(s, offsets[f]), _f64(s, f_deltas[f]))
            hk = s.chest_smooth(hk) if k.chest_mode == cc.WLS else hk
            coded = s.rx_demod(captures_dev(s, x32), D, first_symbol=10, offset=_i32(s, offsets[f]), f_delta=_f64(s, f_deltas[f]), hk=hk)
            coded = bytes(coded[0].cpu().numpy())[16:16 + len(body)]
            n = assert_bytes_match(pad + coded, pad + body, soft, k.mod, what=f"{k.id} frame {f} (coded stream)")
            assert n > 0 and got == rr.hard_finish(orc, 1, coded), f
            excused += n
        st, data = rr.outer_layers(k.ecc, 0, got)
        want[f] = (st, len(data), data)
    return want, excused


def captures_dev(c, x32):
    return c.to_device(np.ascontiguousarray(x32).reshape(1, -1))


def _i32(c, v):
    return torch.tensor([int(v)], dtype=torch.int32, device=c.device)


def _f64(c, v):
    return torch.tensor([float(v)], dtype=torch.float64, device=c.device)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[k.id for k in CASES])
def test_row(orc, index):
    api = _api()
    k = CASES[index]
    seed = cc.seed_of(orc, index)
    assert seed is not None
    ln = cc.link(orc, index, seed)
    D = ln.D
    kw = k.context_kw()
    c = api.Context(**kw)
    s = _stage_context(k.n, k.mod, k.guard)
    ci = api.Context(**{**kw, "ecc": k.inner}) if k.outer and k.inner in rr.HARD_INNER else c
    traces = DISPATCH.setdefault(index, [])

    # ---- transmit
    tx = c.encode_batch(c.to_device(ln.pay))
    c.synchronize()
    traces.append(c.last_dispatch())
    assert tuple(tx.shape) == ln.tx.shape == (cc.FRAMES, (10 + D) * k.S) and D == c.data_symbols(k.payload)
    assert c.coded_len(k.payload) == len(rr.mode_encode(k.ecc, bytes(ln.pay[0])))
    got_tx = tx.cpu().numpy()
    for f in range(cc.FRAMES):
        assert rel_err(got_tx[f], ln.tx[f]) <= 1e-5, (f, rel_err(got_tx[f], ln.tx[f]))

    # ---- front end
    rx = c.to_device(ln.rx)
    r = c.decode_batch(rx, max_symbols=D, n_lags=k.n_lags)
    c.synchronize()
    traces.append(c.last_dispatch())
    h = _host(r)
    fe = cc.reference_front(orc, index, seed)
    for f, w in enumerate(fe):
        assert w.status == 0                                             # (the seed's condition)
        assert int(h["offset"][f]) == w.offset, (f, h["offset"][f], w.offset)
        assert abs(float(h["f_delta"][f]) - w.f_delta) <= 1e-9, (f, h["f_delta"][f], w.f_delta)
        if k.sync_mode == cc.REFERENCE:
            assert abs(float(h["metric"][f]) - w.metric) <= 1e-5 * w.metric, (f, h["metric"][f], w.metric)
        else:
            assert abs(float(h["metric"][f]) - w.metric) <= 1e-6 * max(1.0, w.metric), (f, h["metric"][f], w.metric)
    status = [w.status for w in fe]
    # the options the row sets are the ones the chain took
    disp, soft = traces[-1], k.inner not in rr.HARD_INNER
    assert ("k_chest_solve" in disp) == (k.chest_mode == cc.WLS), disp
    assert ("k_noise_bins" in disp) == ("k_sym<llrw>" in disp) == (soft and k.llr_weight == cc.LLRW_NOISE), disp
    assert ("k_cfo_wide" in disp) == (k.cfo_mode == cc.CFO_WIDE) and ("k_xcorr" in disp) == (k.sync_mode == cc.REFERENCE), disp
    assert ("k_freq_corr" in disp) == (k.sync_mode == cc.REFERENCE and k.cfo_mode != cc.CFO_OFF), disp

    # ---- what the row must deliver
    if k.inner in rr.HARD_INNER:
        hi = h
        if ci is not c:
            hi = _host(ci.decode_batch(rx, max_symbols=D, n_lags=k.n_lags))
            for key in ("offset", "f_delta", "metric"):
                assert np.array_equal(hi[key], h[key]), key              # the outer layers touch nothing of the front end
        want, EXCUSED[index] = _hard_rows(orc, k, s, hi, ln.rx, h["offset"], h["f_delta"], status, D)
        print(f"row {index} {k.id}: excused decisions {EXCUSED[index]}")
    else:
        want = rr.compose(s, rx, k, status, r["offset"], r["f_delta"], D)
    assert_rows_are(r, want)
    # a front-end status of 0 may still end as a frame the mode reports; the front end's own failures are the reference's
    LIVE[index] = [st == 0 and _delivers(k, data, ln.pay[f]) for f, (st, _, data) in sorted(want.items())]

    # ---- a soft mode at its edge: the captures under heavy noise, where every LLR bears on the bytes; the front end's word is the chain's
    if soft:
        noisy = c.to_device(cc.stressed(orc, index, seed))
        rn = c.decode_batch(noisy, max_symbols=D, n_lags=k.n_lags)
        c.synchronize()
        st_n = [st if st in (rr.FRAME_SHORT, rr.FRAME_NOSYNC, rr.FRAME_BADTIMING) else 0 for st in rn["status"].tolist()]
        want_n = rr.compose(s, noisy, k, st_n, rn["offset"], rn["f_delta"], D)
        assert_rows_are(rn, want_n)
        STRESS[index] = [(st, st == 0 and _delivers(k, data, ln.pay[f])) for f, (st, _, data) in sorted(want_n.items())]

    # ---- the other entry points
    before = set(api._CTX_CACHE)
    opts = {key: v for key, v in kw.items() if key not in ("n_fft", "modulation", "guard_bands", "ecc")}
    # (api.decode demodulates every symbol of the capture: the same bytes only behind a length that arrived whole)
    r0, ones = assert_entry_points_agree(api, c, rx, D, decode_kw=dict(ecc=k.ecc, **opts) if all(LIVE[index]) else None)
    traces.append(c.last_dispatch())
    for key in set(api._CTX_CACHE) - before:                            # (api.decode's context: not kept for the rest of the run)
        api._CTX_CACHE.pop(key).close()
    if k.n_lags:
        assert_same_rows(r, c.decode_host(ln.rx, max_symbols=D, n_lags=k.n_lags, chunk_frames=2))
        if all(w.d_hat < k.n_lags - 1 for w in fe):                      # a maximum inside the bound is the search's own: the same rows
            assert_same_rows(r, r0)
    else:
        assert_same_rows(r, r0)
    q, scale = sc16_ref.quantise(ln.rx, 0.9)
    widened = c.to_device(sc16_ref.widen(q, scale))
    qd = c.to_device(q)
    a = c.decode_batch_sc16(qd, max_symbols=D, n_lags=k.n_lags, scale=float(scale))
    traces.append(c.last_dispatch())
    assert_same_rows(a, c.decode_batch(widened, max_symbols=D, n_lags=k.n_lags))
    for f in range(cc.FRAMES):
        one = c.decode_long_sc16(qd[f].contiguous(), D, scale=float(scale))
        two = c.decode_long(widened[f].contiguous(), D)
        assert {key: one[key] for key in ("status", "len", "offset", "f_delta", "metric")} == \
               {key: two[key] for key in ("status", "len", "offset", "f_delta", "metric")}, f
        assert bytes(one["bytes"][:one["len"]].cpu().numpy()) == bytes(two["bytes"][:two["len"]].cpu().numpy()), f
    traces.append(c.last_dispatch())

    # ---- the three captures end to end: one scan, one batched decode
    if k.sync_mode == cc.SC:
        cap = np.ascontiguousarray(ln.rx.reshape(-1))
        cap_dev = c.to_device(cap)
        det = c.sc_scan_long(cap_dev, c.frame_samples(k.payload) - k.reps * k.S, 8)
        traces.append(c.last_dispatch())
        assert len(det["d_hat"]) == cc.FRAMES and not det["more"], det["d_hat"]
        pk = c.decode_packets(cap_dev, det, D)
        c.synchronize()
        traces.append(c.last_dispatch())
        hp = _host(pk)
        geo = [P.geometry(cap.size, k.S, k.backoff, int(d), D) for d in det["d_hat"]]
        prep = [P.prepare(g.length, g.d_rel, k.S, k.backoff, D, k.bytes_per_symbol) for g in geo]
        assert [int(v) for v in hp["offset"]] == [g.r + p.off for g, p in zip(geo, prep)]
        assert all(p.status == 0 for p in prep)
        assert hp["metric"].view(np.int32).tolist() == det["metric"].view(np.int32).tolist()
        if k.cfo_mode != cc.CFO_WIDE:
            assert hp["f_delta"].tolist() == [P.cfo_through(float(v), k.cfo_mode) for v in det["f_delta"]]
        R = P.row_samples(cap.size, k.S, D)
        rows = np.zeros((cc.FRAMES, R), np.complex64)
        for i, g in enumerate(geo):
            rows[i, :g.row_len] = cap[g.r:g.r + g.row_len]
        offs = np.array([p.off for p in prep], np.int32)
        if k.inner in rr.HARD_INNER:
            hpi = hp if ci is c else _host(ci.decode_packets(cap_dev, det, D))
            want_p, n = _hard_rows(orc, k, s, hpi, rows, offs, hp["f_delta"], [0] * cc.FRAMES, D)
            EXCUSED[index] += n
        else:
            want_p = rr.compose(s, c.to_device(rows), k, [0] * cc.FRAMES, c.to_device(offs), pk["f_delta"], D)
        assert_rows_are(pk, want_p)

    print(f"row {index} {k.id} seed {seed}: live {sum(LIVE[index])}/3" + (f", under heavy noise {STRESS[index]}" if soft else "") + "; " + " | ".join(traces))
    assert sum(LIVE[index]) >= 2, LIVE[index]


def test_context_refuses_every_excluded_pair():
    """what tests/test_cover_cpu.py asserts of ofdm_create, with a device behind it"""
    api = _api()
    base = dict(n_fft=64, modulation=2, guard_bands=True)
    for pair in cc.excluded_pairs():
        d = dict(pair)
        kw = {name: d[name] for name in ("sync_mode", "cfo_mode") if name in d}
        if "inner" in d:
            kw["ecc"] = d["inner"] + d["outer"]
        if "sync_backoff" in d:
            kw["sync_backoff"] = 16
        with pytest.raises(api.OfdmError):
            api.Context(**base, **kw)
    with pytest.raises(api.OfdmError):
        api.Context(**base, chest_mode=api.CHEST_WLS, sync_backoff=12)
    api.Context(**base, chest_mode=api.CHEST_WLS, sync_backoff=11).close()
    api.Context(**base, chest_mode=api.CHEST_WLS, sync_backoff=16, sync_mode=api.SYNC_REFERENCE).close()


def test_liveness_and_dispatch_across_the_table():
    """(over the rows this run decoded) nine frames in ten deliver their payload in the reference; the kernels the cover reached"""
    frames = [v for live in LIVE.values() for v in live]
    names = sorted({name for traces in DISPATCH.values() for t in traces for name in t.split("+") if name})
    print(f"{len(LIVE)} rows, {sum(frames)} of {len(frames)} frames delivered; excused decisions {sum(EXCUSED.values())}")
    noisy = [v for rows in STRESS.values() for v in rows]
    print(f"under heavy noise: {len(noisy)} frames of soft rows, {sum(st == 0 for st, _ in noisy)} with status 0, {sum(ok for _, ok in noisy)} delivered")
    print("kernels reached: " + " ".join(names))
    assert not frames or sum(frames) >= 0.9 * len(frames)
