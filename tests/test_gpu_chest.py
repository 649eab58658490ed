"""GPU checks of EXT-5, channel-estimate denoising (include/ofdm_hip.h; definition: tests/chest_ref.py): the stage
ofdm_chest_smooth_batch (k_chest_weight + k_sym<ifft> + k_chest_solve + k_sym<fft>) against the f64 definition, the wiring of
chest_mode = OFDM_CHEST_WLS into ofdm_estimate_channel_batch and into every decode entry point, and what the mode buys on the
captures of tests/chest_cases.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_refs  # noqa: E402
import chest_cases as cc  # noqa: E402
import chest_ref as cr  # noqa: E402
import framed_ref as fr  # noqa: E402
import rs_vectors as rv  # noqa: E402
from chain_checks import assert_entry_points_agree, assert_rows_are, ofdm_api as _api  # noqa: E402
from tools.link import link  # noqa: E402
from util import assert_bytes_match, header_rule, rel_err, wide  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 67


# ---------------------------------------------------------------------------------------------------------- 1. the stage
@functools.lru_cache(maxsize=None)
def _stage_case(n_fft):
    """(rows complex64 [67, n_fft], f64 definition of the same rows, tolerance): 33 oracle LS estimates of a frame through the
    oracle's channel at 30 dB and 33 at 14 dB (one channel seed each), and the bare H = 1.  Computed once per n_fft."""
    from oracle import oracle as orc

    S = n_fft + n_fft // 4
    trn = orc.default_training(n_fft)
    tx = orc.encode(b"EXT-5", guard=True, modulation=6, n_fft=n_fft)
    off = None
    rows = []
    for i in range(ROWS - 1):
        rx, _ = orc.channel(tx, 30.0 if i % 2 == 0 else 14.0, False, 500 + i)
        if off is None:
            off = orc.decode_sc(rx, guard=True, modulation=6, n_fft=n_fft)["offset"]
        rows.append(orc.estimate_channel(rx[off + 5 * S:off + 10 * S], trn, n_fft))
    rows.append(np.ones(n_fft, np.complex128))
    rows = np.asarray(rows).astype(np.complex64)
    want = cr.smooth(wide(rows), trn, n_fft)
    c64 = cr.smooth_c64(rows, trn, n_fft)
    measured = max(rel_err(c64[r], want[r]) for r in range(ROWS))
    return rows, want, measured, max(4.0 * measured, 1e-5)


@pytest.mark.parametrize("n_frames", [1, 3, ROWS])
@pytest.mark.parametrize("n_fft", [64, 128, 1024, 4096])
def test_stage_matches_the_definition(n_fft, n_frames):
    api = _api()
    rows, want, measured, tol = _stage_case(n_fft)
    pick = {1: [ROWS - 2], 3: [0, 1, ROWS - 1]}.get(n_frames, list(range(ROWS)))      # (the H = 1 row is in the 3 and in the 67)
    c = api.Context(n_fft=n_fft)
    assert c.chest_window() == (-(n_fft // 16), n_fft // 4) == cr.window(n_fft)
    x = c.to_device(rows[pick])
    got = c.chest_smooth(x)
    c.synchronize()
    assert "k_chest_solve" in c.last_dispatch() and c.last_dispatch().startswith("k_chest_weight")
    g = got.cpu().numpy()
    err = max(rel_err(g[i], want[r]) for i, r in enumerate(pick))
    print(f"n_fft {n_fft}, {n_frames} rows: complex64 restatement {measured:.2e}, kernel {err:.2e}, allowed {tol:.2e}")
    assert err <= tol
    for cap in (1, 3):                                     # many tiles per workgroup: the same bytes
        c.set_tuning("grid_cap", cap)
        assert torch.equal(c.chest_smooth(x), got), cap
    c.set_tuning("grid_cap", 0)
    y = x.clone()
    assert c.chest_smooth(y, out=y) is y and torch.equal(y, got)                     # in place
    z = c.chest_smooth(x)
    c.synchronize()
    assert torch.equal(z, got) and torch.equal(x.cpu(), torch.from_numpy(rows[pick]))   # (the input is left alone)


def test_stage_argument_checks():
    api = _api()
    c = api.Context(n_fft=64)
    x = c.to_device(np.ones((2, 64), np.complex64))
    f = c.lib.ofdm_chest_smooth_batch
    assert f(c.h, None, 2, x.data_ptr()) == -1 and f(c.h, x.data_ptr(), 2, None) == -1 and f(c.h, x.data_ptr(), -1, x.data_ptr()) == -1
    assert f(c.h, None, 0, None) == 0
    # a training table with too few live bins for cp_len taps: the stage refuses, and so does a context that asks for the mode
    trn = np.zeros(64, np.complex128)
    trn[:10] = 1.0
    dead = api.Context(n_fft=64, training=trn)
    assert f(dead.h, x.data_ptr(), 2, x.data_ptr()) == -1
    with pytest.raises(api.OfdmError):
        api.Context(n_fft=64, training=trn, chest_mode=api.CHEST_WLS)


# ---------------------------------------------------------------------------------------------------------- 2. the mode's wiring
def _link(ecc, n, n_frames, payload, seed, chest_mode, mod=4, snr=30.0):
    """the seeded link of tools/link.py with guard bands and the context's chest_mode set"""
    return link(ecc, n, mod, n_frames, payload, snr, seed, chest_mode=chest_mode)


@pytest.mark.parametrize("n", [64, 1024])
def test_estimate_channel_with_the_mode_is_the_stage_of_the_plain_estimate(n):
    api = _api()
    on, _, rx, _ = _link(api.ECC_NONE, n, 5, 100, 3, api.CHEST_WLS)
    off = api.Context(n_fft=n, modulation=4, guard_bands=True)
    d, fd, _ = off.sc_correlate(rx)
    offs = torch.clamp(d - off.S - 4, min=0).to(torch.int32)
    h_on = on.estimate_channel(rx, offs, fd)
    assert "k_chest_solve" in on.last_dispatch()
    h_ls = off.estimate_channel(rx, offs, fd)
    assert "k_chest" not in off.last_dispatch()
    assert torch.equal(h_on, off.chest_smooth(h_ls)) and torch.equal(h_on, on.chest_smooth(h_ls))
    assert not torch.equal(h_on, h_ls)


def _staged_reference(c, rx, r, D, ecc, orc):
    """{frame: (status, out_len, bytes)} from the staged calls on the same context with the chain's own timing"""
    api = _api()
    if ecc == api.ECC_HAMMING74_SOFT:
        return {f: (0, n, b) for f, (n, b) in chain_refs.soft_reference_decode(c, rx, r, D).items()}
    if ecc == api.ECC_CONV_K7:
        return {f: (0, n, b) for f, (n, b) in chain_refs.conv_reference_decode(c, rx, r, D).items()}
    body = D * c.bytes_per_symbol - 16
    hard, L = chain_refs.hard_and_llrs(c, rx, r, D, want_llr=ecc == api.ECC_CONV_K7F_R34)
    want = {}
    for f in range(rx.shape[0]):
        st = int(r["status"][f])
        if ecc == api.ECC_CONV_K7F_R34:
            if st in (0, fr.HEADER_STATUS):
                s, data = fr.decode_stream(L[f, 128:128 + 8 * body], body, 2)
                want[f] = (s, len(data), data)
            continue
        if st != 0:
            continue
        keep = header_rule(*chain_refs.header_of(hard[f]), body)
        data = bytes(hard[f, 16:16 + keep])
        want[f] = (0, keep, data) if ecc == api.ECC_NONE else (0, keep // 7 * 4, orc.hamming74_decode(data[:keep // 7 * 7])[0])
    return want


@pytest.mark.parametrize("ecc_name", ["ECC_NONE", "ECC_HAMMING74", "ECC_HAMMING74_SOFT", "ECC_CONV_K7", "ECC_CONV_K7F_R34", "ECC_RS255_K7F_R34"])
@pytest.mark.parametrize("n", [64, 128, 1024])
def test_chain_with_the_mode_is_the_composition_of_the_stages(orc, n, ecc_name):
    api = _api()
    ecc = getattr(api, ecc_name)
    # ofdm_channel_batch scales its noise by the whole frame's variance: at N = 1024 the data symbols see about 12 dB less than
    # snr_db, so the link there carries QPSK, the shorter ones 16-QAM -- every coded mode then delivers its payload
    mod = api.QPSK if n == 1024 else api.QAM16
    c, pay, rx, D = _link(ecc, n, 5, 300, 40 + n, api.CHEST_WLS, mod=mod)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    assert "k_chest_solve" in c.last_dispatch() and "k_rxframe" not in c.last_dispatch()
    status = r["status"].cpu().numpy()
    # the timing the chain reports is the search's own
    d, fd, _ = c.sc_correlate(rx)
    assert torch.equal(r["offset"], torch.clamp(d - c.S - 4, min=0).to(torch.int32)) and torch.equal(r["f_delta"], fd)
    if ecc == api.ECC_RS255_K7F_R34:                       # the host RS decoder over what the inner mode's context delivers
        inner = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc - 20, chest_mode=api.CHEST_WLS)
        ri = inner.decode_batch(rx, max_symbols=D)
        inner.synchronize()
        ist, iln, iby = ri["status"].cpu().numpy(), ri["len"].cpu().numpy(), ri["bytes"].cpu().numpy()
        want = {}
        for f in range(rx.shape[0]):
            if ist[f] != 0:
                want[f] = (int(ist[f]), 0, b"")
                continue
            data, out_len, fixed = rv.host_row(c.lib, iby[f], int(iln[f]))
            want[f] = (chain_refs.UNCORRECTABLE, 0, b"") if fixed < 0 else (0, out_len, data)
    else:
        want = _staged_reference(c, rx, r, D, ecc, orc)
    assert sum(1 for st, _, _ in want.values() if st == 0) >= 3
    assert_rows_are(r, want)
    good = [f for f, (st, n_out, data) in want.items() if st == 0 and bytes(data[:300]) == bytes(pay[f].cpu().numpy())]
    if ecc != api.ECC_NONE and ecc != api.ECC_HAMMING74:
        assert len(good) >= 3                              # (30 dB: the coded modes deliver the payload)
    if ecc == api.ECC_NONE:
        # the hard bytes are the oracle's, given the device's H', offset and CFO
        hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
        hard = c.rx_demod(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
        c.synchronize()
        S = c.S
        for f in range(rx.shape[0]):
            if status[f] != 0:
                continue
            x = np.concatenate([wide(rx[f].cpu().numpy()), np.zeros((10 + D) * S, np.complex128)])
            o = int(r["offset"][f])
            rot = orc.cfo_rotate(x[o:o + (10 + D) * S], float(r["f_delta"][f]), 0)
            ob, soft = orc.rx_demod(rot[10 * S:], n, True, mod, hk=wide(hk[f].cpu().numpy()), want_soft=True)
            assert_bytes_match(bytes(hard[f].cpu().numpy()), ob, soft, mod, what=f"frame {f}")


def test_every_decode_entry_point_with_the_mode():
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7F_R34, 64, 5, 300, 91, api.CHEST_WLS)
    r, ones = assert_entry_points_agree(api, c, rx, D)      # (api.decode builds its own context: it has no chest_mode to pass on)
    assert int((r["status"] == 0).sum()) >= 3
    cap = rx[1].contiguous()
    st, n_out, off, data = ones[1]
    d_hat = int(c.sc_correlate(cap.reshape(1, -1))[0][0])
    assert d_hat > 1      # (lag_lo = 1 leaves the detection where it is and takes the route of a known timing)
    for res in (c.decode_long(cap, D, d_hat_known=d_hat), c.decode_long(cap, D, lag_lo=1)):
        assert (res["status"], res["len"], res["offset"]) == (st, n_out, off)
        assert bytes(res["bytes"].cpu().numpy()[:n_out]) == data
    assert "k_chest_solve" in c.last_dispatch()
    assert n_out == 300 and data == bytes(pay[1].cpu().numpy())


@pytest.mark.parametrize("n", [64, 1024])
def test_dispatch_shows_the_solve_only_with_the_mode(n):
    api = _api()
    for ecc in (api.ECC_NONE, api.ECC_HAMMING74_SOFT):
        on, _, rx, D = _link(ecc, n, 4, 100, 7, api.CHEST_WLS)
        off = api.Context(n_fft=n, modulation=4, guard_bands=True, ecc=ecc)
        on.decode_batch(rx, max_symbols=D)
        off.decode_batch(rx, max_symbols=D)
        assert "k_chest_weight" in on.last_dispatch() and "k_chest_solve" in on.last_dispatch() and "k_rxframe" not in on.last_dispatch()
        assert "k_chest" not in off.last_dispatch()
        assert ("k_rxframe" in off.last_dispatch()) == (ecc == api.ECC_NONE)      # the default chain is the one it was


# ---------------------------------------------------------------------------------------------------------- 3. what it buys
def test_mode_earns_its_keep_on_the_1024_carrier_captures(orc):
    """N = 1024, 64-QAM, guard bands, 28 dB, the six frames of tests/chest_cases.py through ofdm_channel_batch (the noise stream
    of orc.channel), decoded with ECC_NONE with the mode off and on.  At this error rate most 16-byte length headers are hit, so
    what decode_batch delivers is cut by a garbled length; the errors are therefore counted on the bytes decode demodulated --
    rx_demod with the chain's own timing and estimate, which the delivered bytes are checked to be a slice of -- over the 16 + 1304
    bytes every frame carries, against the oracle's noiseless demodulation: the count the oracle makes for the same H rule."""
    api = _api()
    n, snr = 1024, 28.0
    caps = cc.captures(n, snr)
    trn = orc.default_training(n)
    pays = torch.from_numpy(cc.payloads(n))
    counts, oracle = {}, {}
    for mode in (api.CHEST_LS, api.CHEST_WLS):
        c = api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, chest_mode=mode)
        tx = c.encode_batch(pays.to(c.device))
        rx = c.channel_batch(tx, snr_db=snr, seed=cc.SEED0)
        D = c.data_symbols(pays.shape[1])
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        assert ("k_chest_solve" in c.last_dispatch()) == (mode == api.CHEST_WLS)
        assert (r["status"] == 0).all()
        hard, _ = chain_refs.hard_and_llrs(c, rx, r, D, want_llr=False)
        total = 0
        for f, cap in enumerate(caps):
            n_out = int(r["len"][f])
            assert bytes(r["bytes"][f, :n_out].cpu().numpy()) == bytes(hard[f, 16:16 + n_out])
            total += int((cc.bits(hard[f, :cap["n_bytes"]]) != cap["ref_bits"]).sum())
        counts[mode] = total
        oracle[mode] = sum(cc.hard_errors(n, cap, cap["h_ls"] if mode == api.CHEST_LS else cr.smooth(cap["h_ls"], trn, n)) for cap in caps)
    print(f"hard bit errors, device: {counts[0]} -> {counts[1]}; oracle: {oracle[0]} -> {oracle[1]}")
    assert (oracle[0], oracle[1]) == (767, 305)
    assert counts[1] < counts[0]
    for mode in counts:
        assert abs(counts[mode] - oracle[mode]) <= 0.02 * oracle[mode], (mode, counts[mode], oracle[mode])
