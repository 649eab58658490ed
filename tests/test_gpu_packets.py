"""GPU checks of ofdm_rx_decode_packets and ofdm_rx_decode_all_long_host (EXT-13: k_pkt_rows + k_gather_rows + the receive chain with
k_rx_prepare_rows + k_pkt_finish) against tests/packets_ref.py -- the row rules in integers and orc.decode_given on capture[r_k:].

  1. the definition on the captures of scan_ref.CAPTURES (and n64_a less its first 6 samples, the one case where the rule's clamp of the
     trimmed start to 0 acts: packets_ref.CASES): status, offset, out_len exact, bytes under util.assert_bytes_match, f_delta and
     metric bit-equal to what went in;
  2. against the loop: decode_long(lag_lo = lo_k) agrees in status, out_len and offset, its f_delta within 1e-9 (bytes are not compared
     with the loop: a CFO 1e-9 apart may move a point across a decision boundary; test 1 holds the bytes);
  3. every mode family on frames of tools/link.py's seeded link laid back to back with unequal gaps, at an SNR where the mode loses
     nothing (the premise is asserted through the decode_long loop first): row k of the batched call is the call with packet k alone,
     bit for bit; grid_cap 1 and 3 and chunks of 2 rows change nothing; the payloads are what was sent;
  4. the row contract: a capture on an 8-byte boundary, an odd out_stride, detections reversed and with a duplicate;
  5. every argument error, n_det = 0, decode_all(batched=True) without max_symbols;
  6. the host form from pageable and pinned memory against the device form, and api.decode_all(batched=True) against decode_all().
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import packets_ref as P
import scan_ref as R
from util import assert_bytes_match

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.link import data_snr, link_on, wide_link_on  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 10 ** 6
MOD = 4
FIELDS = ("len", "status", "offset", "f_delta", "metric")


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def host(ctx, res):
    ctx.synchronize()
    return {k: res[k].cpu().numpy() if hasattr(res[k], "cpu") else res[k] for k in ("bytes",) + FIELDS}


def packet_of(r, k):
    """everything the call delivered for packet k, floats as their bit patterns"""
    n = int(r["len"][k]) if int(r["status"][k]) == 0 else 0
    return (int(r["status"][k]), int(r["len"][k]), int(r["offset"][k]), np.float64(r["f_delta"][k]).view(np.int64).item(),
            np.float32(r["metric"][k]).view(np.int32).item(), bytes(r["bytes"][k, :max(n, 0)]))


def all_packets(r):
    return [packet_of(r, k) for k in range(len(r["status"]))]


def sub(det, idx):
    return {k: np.ascontiguousarray(np.asarray(det[k])[idx]) for k in ("d_hat", "f_delta", "metric")}


# ---------------------------------------------------------------------------------------------------------- 1 + 2: the definition
def scanned(api, orc, name):
    b = P.built(orc, name)
    ctx = api.Context(n_fft=b.n_fft, modulation=api.QAM16, guard_bands=True, sync_threshold=R.THRESHOLD)
    x = ctx.to_device(b.x)
    det = ctx.sc_scan_long(x, min(b.frame_samples) - b.W, ALL)
    assert det["d_hat"].size == len(b.frame_samples) and not det["more"]
    return b, ctx, x, det


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_packets_are_the_definition(api, orc, name):
    b, ctx, x, det = scanned(api, orc, name)
    D = P.CASES[name]
    got = host(ctx, ctx.decode_packets(x, det, D))
    disp = ctx.last_dispatch()
    assert "k_pkt_rows" in disp and "k_gather_rows" in disp and "k_rx_prepare_rows" in disp and disp.endswith("k_pkt_finish"), disp
    want = P.packets(orc, b.x, det, b.n_fft, True, MOD, D)
    for k, w in enumerate(want):
        what = (name, k)
        assert (int(got["status"][k]), int(got["offset"][k]), int(got["len"][k])) == (w["status"], w["offset"], w["len"]), (what, w["status"], w["offset"], w["len"])
        if w["status"] == 0:
            assert_bytes_match(bytes(got["bytes"][k, : w["len"]]), w["bytes"], w["soft"][128 // MOD:], MOD, what=str(what))
    assert got["f_delta"].view(np.int64).tolist() == det["f_delta"].view(np.int64).tolist()      # CFO_SIGNED: what the chain derotated with
    assert got["metric"].view(np.int32).tolist() == det["metric"].view(np.int32).tolist()
    # the frame at sample 0 (the trimmed start clamped to 0 in the capture cut by 6 samples) and the last frame, cut by the capture's end
    assert P.first_is_clamped(b, det["d_hat"]) == name.endswith("_cut6")
    assert int(got["offset"][0]) == (0 if name.endswith("_cut6") else 5) and int(got["status"][0]) == 0
    assert P.last_is_cut(b, want[-1]) and (int(got["status"][-1]) == api.FRAME_SHORT or want[-1]["ns"] < D)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_packets_against_the_loop(api, orc, name):
    b, ctx, x, det = scanned(api, orc, name)
    D = P.CASES[name]
    got = host(ctx, ctx.decode_packets(x, det, D))
    for k in range(det["d_hat"].size):
        one = ctx.decode_long(x, D, lag_lo=int(det["lag_lo"][k]))
        assert (one["status"], one["len"], one["offset"]) == (int(got["status"][k]), int(got["len"][k]), int(got["offset"][k])), (name, k)
        assert abs(one["f_delta"] - float(got["f_delta"][k])) <= 1e-9, (name, k, one["f_delta"], float(got["f_delta"][k]))


# ---------------------------------------------------------------------------------------------------------- 3: every mode family
GAPS = (0, 37, 402, 3, 1211, 90, 15, 700)              # samples of silence in front of frame f (the link's own 1 .. 32 come on top)


def laid_out(ctx, rx):
    """the link's captures [n_frames, span] back to back with the gaps above -> one capture on the device, zeros in the gaps and 500
    samples behind the last frame"""
    import torch

    n_frames, span = rx.shape
    at, pos = [], 0
    for f in range(n_frames):
        pos += GAPS[f % len(GAPS)] * (ctx.S // 80)
        at.append(pos)
        pos += span
    cap = torch.zeros(pos + 500, dtype=torch.complex64, device=ctx.device)
    for f, st in enumerate(at):
        cap[st: st + span] = rx[f]
    return cap, at


# key -> (n_fft, modulation, ecc, frames, payload bytes, snr of the link, context options, wide CFO link)
def _families(api):
    coded = dict(n=64, mod=api.QPSK, frames=8, payload=120, snr=25.0, kw={}, wide=False)
    fam = {
        "none": dict(coded, mod=api.QAM16, ecc=api.ECC_NONE, snr=30.0),
        "hamming74": dict(coded, ecc=api.ECC_HAMMING74),
        "hamming74_soft": dict(coded, ecc=api.ECC_HAMMING74_SOFT),
        "conv_k7f_r34": dict(coded, ecc=api.ECC_CONV_K7F_R34),
        "rs255_k7f_r34": dict(coded, ecc=api.ECC_RS255_K7F_R34),
        "ldpc648": dict(coded, ecc=api.ECC_LDPC648),
        "fcs_ldpc648_r34": dict(coded, ecc=api.ECC_FCS + api.ECC_LDPC648_R34),
        "chest_wls": dict(coded, mod=api.QAM16, ecc=api.ECC_NONE, snr=30.0, kw=dict(chest_mode=api.CHEST_WLS)),
        "cfo_wide": dict(coded, ecc=api.ECC_CONV_K7F_R34, kw=dict(cfo_mode=api.CFO_WIDE), wide=True),
        "llrw_noise": dict(coded, ecc=api.ECC_LDPC648, kw=dict(llr_weight=api.LLRW_NOISE)),
        # N = 1024: the fused frame kernel with its Hamming finish, and the generic soft chain (30 dB at the data symbols, data_snr)
        "n1024_hamming74": dict(coded, n=1024, ecc=api.ECC_HAMMING74, frames=3, payload=900, snr=float(data_snr(1024, 30.0))),
        "n1024_hamming74_soft": dict(coded, n=1024, ecc=api.ECC_HAMMING74_SOFT, frames=3, payload=900, snr=float(data_snr(1024, 30.0))),
    }
    return fam


FAMILIES = ("none", "hamming74", "hamming74_soft", "conv_k7f_r34", "rs255_k7f_r34", "ldpc648", "fcs_ldpc648_r34", "chest_wls", "cfo_wide",
            "llrw_noise", "n1024_hamming74", "n1024_hamming74_soft")


def family_capture(api, key, seed=1300):
    f = _families(api)[key]
    ctx = api.Context(n_fft=f["n"], modulation=f["mod"], guard_bands=True, ecc=f["ecc"], **f["kw"])
    if f["wide"]:
        pay, rx, _, _ = wide_link_on(ctx, f["frames"], f["payload"], f["snr"], seed + f["ecc"])
    else:
        pay, rx = link_on(ctx, f["frames"], f["payload"], f["snr"], seed + f["ecc"])
    cap, at = laid_out(ctx, rx)
    holdoff = ctx.frame_samples(f["payload"]) - ctx.params.sync_window_reps * ctx.S
    return ctx, f, pay.cpu().numpy(), cap, at, holdoff, ctx.data_symbols(f["payload"])


def delivered_payloads(r, pay):
    return all(int(r["status"][k]) == 0 and int(r["len"][k]) >= pay.shape[1] and bytes(r["bytes"][k, : pay.shape[1]]) == bytes(pay[k])
               for k in range(pay.shape[0]))


@pytest.mark.parametrize("key", FAMILIES)
def test_packets_batch_grid_and_chunk_independence(api, key):
    ctx, f, pay, cap, at, holdoff, D = family_capture(api, key)
    det = ctx.sc_scan_long(cap, holdoff, ALL)
    assert det["d_hat"].size == f["frames"], (key, det["d_hat"], at)
    # the premise, through the existing loop: every whole frame yields its payload
    for k in range(f["frames"]):
        one = ctx.decode_long(cap, D, lag_lo=int(det["lag_lo"][k]))
        assert one["status"] == 0 and one["len"] >= f["payload"] and bytes(one["bytes"][: f["payload"]].cpu().numpy()) == bytes(pay[k]), (key, k, one["status"])
    whole = host(ctx, ctx.decode_packets(cap, det, D))
    disp = ctx.last_dispatch()
    assert "k_gather_rows" in disp, disp
    if key == "none":
        assert "k_rxframe64" in disp, disp
    if key == "n1024_hamming74":
        assert "k_rxframe1024" in disp, disp
    assert delivered_payloads(whole, pay), (key, whole["status"], whole["len"])
    assert all(0 <= int(whole["offset"][k]) - at[k] < 2 * ctx.S for k in range(f["frames"]))
    want = all_packets(whole)
    for k in range(f["frames"]):                                        # packet k alone
        alone = host(ctx, ctx.decode_packets(cap, sub(det, [k]), D))
        assert packet_of(alone, 0) == want[k], (key, k)
    for tune in ({"grid_cap": 1}, {"grid_cap": 3}, {"packets_chunk_rows": 2}):
        for name, v in tune.items():
            ctx.set_tuning(name, v)
        assert all_packets(host(ctx, ctx.decode_packets(cap, det, D))) == want, (key, tune)
        assert "k_gather_rows" in ctx.last_dispatch()
        for name in tune:
            ctx.set_tuning(name, 0)


# ---------------------------------------------------------------------------------------------------------- 4: the row contract
def test_packets_row_contract(api):
    import torch

    ctx, f, pay, cap, at, holdoff, D = family_capture(api, "none")
    det = ctx.sc_scan_long(cap, holdoff, ALL)
    base = host(ctx, ctx.decode_packets(cap, det, D))
    want = all_packets(base)
    assert delivered_payloads(base, pay) and cap.data_ptr() % 16 == 0
    # a capture whose base is only 8-byte aligned: a view one sample in
    hold = torch.zeros(cap.numel() + 1, dtype=torch.complex64, device=ctx.device)
    hold[1:] = cap
    view = hold[1:]
    assert view.data_ptr() % 16 == 8
    assert all_packets(host(ctx, ctx.decode_packets(view, det, D))) == want
    assert "k_gather_rows" in ctx.last_dispatch() and "k_rxframe64" in ctx.last_dispatch()
    # an odd out_stride (the fused finish needs dword rows: the chain's own k_rx_finish writes them)
    odd = ctx.decode_row_bytes(D) | 1
    assert odd % 2 == 1
    assert all_packets(host(ctx, ctx.decode_packets(cap, det, D, out_stride=odd))) == want
    # detections in reverse order and with a duplicate: a row is its own triple's
    idx = list(range(f["frames"]))[::-1] + [2, 2]
    got = all_packets(host(ctx, ctx.decode_packets(cap, sub(det, idx), D)))
    assert got == [want[k] for k in idx]


# ---------------------------------------------------------------------------------------------------------- 5: arguments
def test_packets_error_codes(api):
    INVALID, UNSUPPORTED = -1, -2
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    x = ctx.to_device(R.noise_capture(4000))
    n, D = x.numel(), 8
    ob = ctx.decode_row_bytes(D)
    out, ln, st = ctx.empty((4, ob), __import__("torch").uint8), ctx.empty((4,), __import__("torch").int32), ctx.empty((4,), __import__("torch").int32)
    dh, fd, m = np.array([100, 900], np.int64), np.zeros(2), np.zeros(2, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    def call(c=ctx, x=x, n=n, nd=2, dh=dh, fd=fd, m=m, D=D, out=out, stride=ob, ln=ln, st=st):
        return c.lib.ofdm_rx_decode_packets(c.h, p(x), n, nd, p(dh), p(fd), p(m), D, p(out), stride, p(ln), p(st), None, None, None)

    assert call() == 0 and "k_gather_rows" in ctx.last_dispatch() and "k_pkt_finish" not in ctx.last_dispatch()    # no offsets wanted
    ctx.synchronize()
    assert call(dh=np.array([100, -1], np.int64)) == INVALID and call(dh=np.array([n, 100], np.int64)) == INVALID
    assert call(dh=np.array([n - 1, 0], np.int64)) == 0
    ctx.synchronize()
    assert st.cpu().numpy()[:2].tolist() == [api.FRAME_SHORT, 0]
    assert call(nd=-1) == INVALID and call(D=0) == INVALID and call(n=-1) == INVALID
    for name in ("x", "dh", "fd", "m", "out", "ln", "st"):
        assert call(**{name: None}) == INVALID, name
    assert call(stride=ob - 1) == INVALID
    assert call(n=2 ** 40 + 1) == UNSUPPORTED
    ref = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True, sync_mode=api.SYNC_REFERENCE)
    assert call(c=ref) == UNSUPPORTED
    assert call(nd=0, dh=None, fd=None, m=None, out=None, ln=None, st=None) == 0 and ctx.last_dispatch() == ""       # no launch
    empty = ctx.decode_packets(x, {"d_hat": [], "f_delta": [], "metric": []}, D)
    assert empty["status"].numel() == 0 and ctx.last_dispatch() == ""
    with pytest.raises(api.OfdmError):
        ctx.decode_packets(x, {"d_hat": [x.numel()], "f_delta": [0.0], "metric": [0.0]}, D)
    with pytest.raises(api.OfdmError):
        api.decode_all(R.noise_capture(4000), True, api.QAM16, batched=True)
    # the host form: the scan's errors and the decode's
    xh = R.noise_capture(4000)
    outh, i32, i64, f64, f32 = np.zeros((4, ob), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4), np.zeros(4, np.float32)
    nd, st2 = C.c_int64(7), np.zeros(4, np.int32)

    def hcall(x=xh, n=4000, holdoff=1, max_det=4, D=D, out=outh, stride=ob, dhat=i64, ndp=C.byref(nd)):
        return ctx.lib.ofdm_rx_decode_all_long_host(ctx.h, p(x), n, 0, 0, holdoff, max_det, D, p(out), stride, p(i32), p(st2), None, p(f64), p(f32),
                                                    None, p(dhat), ndp, None)

    assert hcall() == 0 and nd.value == 0
    assert hcall(holdoff=0) == INVALID and hcall(max_det=-1) == INVALID and hcall(x=None) == INVALID and hcall(dhat=None) == INVALID
    assert hcall(ndp=None) == INVALID and hcall(D=0) == INVALID and hcall(out=None) == INVALID and hcall(stride=ob - 1) == INVALID
    assert hcall(n=2 ** 40 + 1) == UNSUPPORTED and hcall(n=0, x=None) == 0


# ---------------------------------------------------------------------------------------------------------- 6: host form, api.decode_all
def test_packets_host_form_and_decode_all(api):
    ctx, f, pay, cap, at, holdoff, D = family_capture(api, "none")
    det = ctx.sc_scan_long(cap, holdoff, ALL, 7, 0)
    dev = host(ctx, ctx.decode_packets(cap, det, D))
    want = all_packets(dev)
    assert delivered_payloads(dev, pay)
    xh = cap.cpu().numpy()
    pin = api.pinned_empty((xh.size,), np.complex64)
    pin[:] = xh
    assert ctx.lib.ofdm_host_is_pinned(pin.ctypes.data, pin.nbytes) == 1
    for src in (xh, pin):                                               # pageable, pinned
        got = ctx.decode_all_host(src, holdoff, 64, D, 7, 0)
        disp = ctx.last_dispatch()
        assert disp.startswith("k_sc_mark+k_sc_walk+k_sc_peaks+k_pkt_rows+k_gather_rows") and disp.endswith("k_pkt_finish"), disp
        assert all_packets(got) == want
        for k in ("d1", "d_hat", "lag_lo"):
            assert np.array_equal(got[k], det[k]), k
        assert got["more"] == det["more"] and got["next_lag_lo"] == det["next_lag_lo"]
    two = ctx.decode_all_host(xh, holdoff, 2, D, 7, 0)                 # max_det stops the scan: two packets, more set
    assert two["more"] and all_packets(two) == want[:2]
    # the laboratory key: k_pkt_rows + k_gather_rows alone, nothing is delivered
    ctx.set_tuning("packets_gather_only", 1)
    ctx.decode_packets(cap, det, D)
    ctx.synchronize()
    assert ctx.last_dispatch() == "k_pkt_rows+k_gather_rows", ctx.last_dispatch()
    ctx.set_tuning("packets_gather_only", 0)
    assert all_packets(host(ctx, ctx.decode_packets(cap, det, D))) == want
    # api.decode_all: the batched path against the loop
    kw = dict(guard_bands=True, modulation=f["mod"], n_fft=64, ecc=f["ecc"], holdoff=holdoff, max_symbols=D)
    loop, batched = api.decode_all(xh, **kw), api.decode_all(xh, batched=True, **kw)
    assert len(loop) == len(batched) == f["frames"] and [g["bytes"] for g in batched] == [bytes(r) for r in pay]
    for a, b in zip(loop, batched):
        assert set(a) == set(b)
        for k in a:
            if k == "f_delta":
                assert abs(a[k] - b[k]) <= 1e-9
            elif k == "metric":
                assert abs(a[k] - b[k]) <= 1e-6
            else:
                assert a[k] == b[k], k
    cut = api.decode_all(xh, batched=True, max_packets=2, **kw)
    assert [g["more"] for g in cut] == [False, True] and [g["bytes"] for g in cut] == [bytes(r) for r in pay[:2]]
