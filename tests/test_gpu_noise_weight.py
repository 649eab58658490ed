"""GPU checks of EXT-11, noise-aware LLR weights (include/ofdm_hip.h "noise-aware LLR weights"; definition: tests/noise_weight_ref.py):
  1. the stage ofdm_rx_noise_bins_batch (k_noise_bins) against the f64 definition at N = 64 .. 4096, with and without CFO, over a
     frame with a non-zero status, one whose fifth training block the capture cuts, one with a tone and a noiseless one; two grids;
  2. gains +-2^20, 2^-20 and -1: q keeps its bits, s is scaled by g^2 exactly;
  3. the stage ofdm_rx_llr_weighted_batch (k_sym<llrw>) by soft_ref.llr_compare with soft_ref's weights times q;
  4. the decode chains under OFDM_LLRW_NOISE against the stages composed by hand, bit for bit; the mode off against a context that
     never heard of it; modes that form no LLRs;
  5. one link with a tone through decode_batch, mode off against on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combine_ref as cb  # noqa: E402
import fcs_ref  # noqa: E402
import framed_ref as fr  # noqa: E402
import ldpc_ref  # noqa: E402
import ldpc_rates_ref as lrr  # noqa: E402
import noise_weight_ref as nw  # noqa: E402
import rs_vectors as rv  # noqa: E402
import soft_ref as sr  # noqa: E402
from chain_checks import assert_entry_points_agree, assert_rows_are, assert_same_rows, ofdm_api as _api  # noqa: E402
from chain_refs import header_of  # noqa: E402
from tools.link import branch_link_on, link_on  # noqa: E402
from util import fc32, make_symbols_np, wide  # noqa: E402

pytestmark = pytest.mark.gpu

# Row-norm-relative error of s against the f64 definition, and the absolute error of q.  Measured on the rows of
# test_noise_bins_against_the_definition (the test prints them): s 1.2e-7 .. 2.9e-7 without CFO, 4.2e-7 .. 6.05e-7 with (the phasor's
# 1.3e-7), q 2.3e-7 .. 1.62e-6.  The bound is 8 x the largest figure of s, the spread the project's other f32-against-f64 bounds leave
# (DESIGN.md section 3, EXT-11), and holds q, absolute, as well
S_TOL = 8 * 6.05e-7
assert S_TOL <= 1e-4


# ---------------------------------------------------------------------------------------------------------- 1. the stage
def _captures(rng, n, cfo):
    """five captures [5, span] fc32 with their offsets, CFOs, statuses and the frame_len: 0 noisy, 1 a non-zero status, 2 its fifth
    training block cut by frame_len, 3 a tone at bin 11.3, 4 noiseless (five identical blocks, no CFO)"""
    S = n + n // 4
    off = np.array([11, 3, 29, 11, 7], np.int32)
    frame_len = 11 + 10 * S + 12
    span = frame_len + 2 * S
    x = (rng.standard_normal((5, span)) + 1j * rng.standard_normal((5, span))) / np.sqrt(2.0)
    blk = (rng.standard_normal((5, S)) + 1j * rng.standard_normal((5, S))) / np.sqrt(2.0)
    for f in range(5):
        for b in range(5, 10):
            x[f, off[f] + b * S:off[f] + (b + 1) * S] = blk[f]
    noise = 0.1 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    noise[4] = 0.0
    x = x + noise
    x[3] += 0.5 * np.exp(2j * np.pi * 11.3 * np.arange(span) / n)
    fd = None
    if cfo:
        fd = rng.uniform(-1.0, 1.0, 5) / S
        fd[4] = 0.0
        x = x * np.exp(1j * fd[:, None] * (np.arange(span)[None, :] - off[:, None]))
    return fc32(x), off, fd, np.array([0, -2, 0, 0, 0], np.int32), frame_len


def _noise_bins(c, x, off, fd, status, frame_len):
    r = c.noise_bins(c.to_device(x), c.to_device(off), None if fd is None else c.to_device(fd), c.to_device(status), frame_len=frame_len)
    assert c.last_dispatch() == "k_noise_bins", c.last_dispatch()
    return r


@pytest.mark.parametrize("cfo", [False, True])
@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
def test_noise_bins_against_the_definition(n, cfo):
    api = _api()
    rng = np.random.default_rng(1100 + n + cfo)
    x, off, fd, status, frame_len = _captures(rng, n, cfo)
    c = api.Context(n_fft=n, modulation=6, guard_bands=True)
    got = _noise_bins(c, x, off, fd, status, frame_len)
    c.set_tuning("grid_cap", 1)
    one = _noise_bins(c, x, off, fd, status, frame_len)
    c.set_tuning("grid_cap", 0)
    c.synchronize()
    assert torch.equal(got["nvar"], one["nvar"]) and torch.equal(got["weight"], one["weight"]), "grid_cap 1 changes the rows"
    s, q = got["nvar"].cpu().numpy().astype(np.float64), got["weight"].cpu().numpy().astype(np.float64)
    ws, wq = nw.noise_bins(wide(x), n, off, fd, status, frame_len)
    assert (ws[[1, 2, 4]] == 0).all() and (wq[[1, 2, 4]] == 1).all() and (wq[[0, 3]] < 1).any(axis=1).all()
    assert (s[[1, 2, 4]] == 0).all() and (q[[1, 2, 4]] == 1).all()           # not tested / noiseless: exactly 0 and exactly 1
    assert wq[3, 11] < 0.05 and q[3, 11] < 0.05                                # the tone's bin is all but switched off
    assert (q >= 0).all() and (q <= 1).all()
    e_s = max(np.linalg.norm(s[f] - ws[f]) / np.linalg.norm(ws[f]) for f in (0, 3))
    e_q = float(np.abs(q - wq).max())
    print(f"N {n} cfo {cfo}: s row-norm-relative error {e_s:.3g}, q absolute error {e_q:.3g}")
    assert e_s <= S_TOL and e_q <= S_TOL, (e_s, e_q)
    # the mean over the bins is link quality's noise_var
    rows = c.rx_quality(c.to_device(x), 0, 10, None, c.to_device(off), None if fd is None else c.to_device(fd), None, c.to_device(status),
                        frame_len=frame_len).cpu().numpy()
    np.testing.assert_allclose(s.mean(axis=1), rows[:, api.Q_NOISE_VAR], rtol=1e-5, atol=0)


def test_noise_bins_arguments():
    api = _api()
    c = api.Context(n_fft=64, modulation=6, guard_bands=True)
    x = torch.zeros((2, 1000), dtype=torch.complex64, device=c.device)
    off = torch.zeros(2, dtype=torch.int32, device=c.device)
    w = torch.empty((2, 64), dtype=torch.float32, device=c.device)
    f = c.lib.ofdm_rx_noise_bins_batch
    assert f(c.h, None, 0, 1000, 1000, None, None, None, None, None) == 0                      # n_frames == 0
    assert f(c.h, None, 2, 1000, 1000, off.data_ptr(), None, None, None, w.data_ptr()) == -1   # no input
    assert f(c.h, x.data_ptr(), 2, 1000, 1000, None, None, None, None, w.data_ptr()) == -1     # no offsets
    assert f(c.h, x.data_ptr(), -1, 1000, 1000, off.data_ptr(), None, None, None, w.data_ptr()) == -1
    assert f(c.h, x.data_ptr(), 2, 1000, 0, off.data_ptr(), None, None, None, w.data_ptr()) == -1
    assert f(c.h, x.data_ptr(), 2, 1000, 1000, off.data_ptr(), None, None, None, w.data_ptr()) == 0   # f_delta, status, nvar optional
    c.synchronize()
    assert bool((w == 1).all())                                                                 # an all-zero capture is noiseless


# ---------------------------------------------------------------------------------------------------------- 2. gain
@pytest.mark.parametrize("n", [64, 1024])
def test_gain_leaves_q_alone_and_scales_s_exactly(n):
    api = _api()
    rng = np.random.default_rng(1200 + n)
    x, off, fd, status, frame_len = _captures(rng, n, True)
    c = api.Context(n_fft=n, modulation=6, guard_bands=True)
    base = _noise_bins(c, x, off, fd, status, frame_len)
    assert bool((base["weight"] < 1).any())
    for g in (2.0 ** 20, -(2.0 ** 20), 2.0 ** -20, -1.0):
        got = _noise_bins(c, fc32(wide(x) * g), off, fd, status, frame_len)
        assert torch.equal(got["weight"], base["weight"]), g
        assert torch.equal(got["nvar"], base["nvar"] * (g * g)), g


# ---------------------------------------------------------------------------------------------------------- 3. weighted LLRs
@pytest.mark.parametrize("mod", [1, 6])
@pytest.mark.parametrize("n", [64, 256])
def test_weighted_llrs_against_the_definition(orc, n, mod):
    api = _api()
    rng = np.random.default_rng(1300 + n + mod)
    F, D = (5, 7) if n == 64 else (5, 3)
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True)
    hk = fc32(1.0 + 0.3 * (rng.standard_normal((F, n)) + 1j * rng.standard_normal((F, n))))
    x, _ = make_symbols_np(orc, rng, F * D, n, True, mod, snr_db=14.0)
    x = sr.through_h(x.reshape(F, -1), n, hk)
    ref = sr.oracle_llr_reference(orc, x, n, True, mod, 32.0, hk)
    bins = sr.data_bins(orc, n, True)
    xd, hd = c.to_device(x), c.to_device(hk)
    plain = c.rx_llr(xd, D, hk=hd)
    assert c.last_dispatch() == "k_sym<llr>"
    # a NULL weight: the bytes and the dispatch of rx_llr
    nl = plain.shape[1]
    null = torch.empty_like(plain)
    f = c.lib.ofdm_rx_llr_weighted_batch
    args = (c.h, xd.data_ptr(), F, xd.shape[1], xd.shape[1], 0, D, None, None, hd.data_ptr(), n, 32.0, null.data_ptr(), nl)
    assert f(*args, None, 0) == 0 and c.last_dispatch() == "k_sym<llr>" and torch.equal(null, plain)
    ones = torch.ones((F, n), dtype=torch.float32, device=c.device)
    assert f(*args, ones.data_ptr(), 7) == -1 and f(*args, ones.data_ptr(), 2 * n) == -1     # the stride is 0 or n_fft
    # all ones: the other kernel, the same bytes
    got = c.rx_llr(xd, D, hk=hd, bin_weight=ones)
    assert c.last_dispatch() == "k_sym<llrw>" and torch.equal(got, plain)
    # a shared row and a row per frame, in (0, 1]
    for what, q in (("shared", rng.uniform(0.02, 1.0, (1, n)).astype(np.float32)), ("per frame", rng.uniform(0.02, 1.0, (F, n)).astype(np.float32))):
        q[:, ::7] = 1.0
        qd = c.to_device(q[0] if what == "shared" else q)
        got = c.rx_llr(xd, D, hk=hd, bin_weight=qd)
        assert c.last_dispatch() == "k_sym<llrw>"
        c.set_tuning("grid_cap", 1)
        assert torch.equal(c.rx_llr(xd, D, hk=hd, bin_weight=qd), got), "grid_cap 1 changes the LLRs"
        c.set_tuning("grid_cap", 0)
        qw = np.broadcast_to(q.astype(np.float64)[:, bins], (F, bins.size))[:, None, :, None]
        shape = (F, D, bins.size, mod)
        y = (ref["y"].reshape(shape) * qw).reshape(F, -1)
        eps = (ref["eps"].reshape(shape) * qw).reshape(F, -1) + np.abs(y) * 2.0 ** -24    # one more f32 rounding: the product with q
        share = sr.llr_compare(got.cpu().numpy(), y, eps, what=f"N {n} mod {mod} {what}")
        print(f"N {n} mod {mod} {what}: excused {100 * share:.3f} %")
        assert share <= 0.02
        assert not torch.equal(got, plain)


# ---------------------------------------------------------------------------------------------------------- 4. the chains
N, MOD, PAYLOAD, FRAMES = 64, 6, 150, 8
TONE, EMPTY = 2, 5                                                  # the frame with a tone on it, the slot without a packet
MODES = [2, 12, 16, 94]                                             # HAMMING74_SOFT, CONV_K7F_R34, LDPC648, FCS + RS255_K7F_R12


def _chain_link(api, ecc, seed, branches=1):
    """(c under LLRW_NOISE, c0 = the front end alone, pay, rx [F, span] or [F, R, span], D)"""
    c = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc, llr_weight=api.LLRW_NOISE)
    c0 = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=api.ECC_NONE)
    pay, rx = branch_link_on(c, FRAMES, PAYLOAD, [22.0 - 3.0 * r for r in range(branches)], seed)   # [F, R, span]
    k = torch.arange(rx.shape[2], device=c.device, dtype=torch.float64)
    g = torch.Generator(device=c.device)
    g.manual_seed(seed + 7)
    for r in range(branches):
        amp = 0.3 * float(rx[TONE, r].abs().pow(2).mean().sqrt())
        rx[TONE, r] += (amp * torch.exp(2j * np.pi * 11.3 * k / N)).to(torch.complex64)
        rx[EMPTY, r] = 1e-3 * torch.randn(rx.shape[2], dtype=torch.complex64, device=c.device, generator=g)
    return c, c0, pay, (rx[:, 0].contiguous() if branches == 1 else rx), c.data_symbols(PAYLOAD)


def _stages(c, c0, rows, D):
    """front-end outputs -> channel estimate -> noise_bins -> rx_llr with the weights (and the hard bytes), through the stage entry
    points; the front end's status, offset and f_delta are decode_batch's on a context without a code"""
    fe = c0.decode_batch(rows, max_symbols=D)
    status = fe["status"]
    off = torch.where(status == 0, fe["offset"], torch.zeros_like(fe["offset"]))
    hk = c.estimate_channel(rows, off, fe["f_delta"])
    nb = c.noise_bins(rows, off, fe["f_delta"], status)
    llr = c.rx_llr(rows, D, first_symbol=10, offset=off, f_delta=fe["f_delta"], hk=hk, bin_weight=nb["weight"])
    assert c.last_dispatch() == "k_sym<llrw>"
    hard = c.rx_demod(rows, D, first_symbol=10, offset=off, f_delta=fe["f_delta"], hk=hk)
    c.synchronize()
    return fe, off, hk, nb, llr, hard


def _finish(c, ecc, st, llr_row, hard_row, body):
    """(status, bytes) of one live frame by the mode's CPU frame rules over its LLR row (and, for the header of mode 2, its hard bytes)"""
    fcs = ecc >= 64
    base = ecc - 64 if fcs else ecc
    rs = base in (30, 31, 32)
    inner = base - 20 if rs else base
    if inner == 2:
        lo, hi = header_of(hard_row)
        keep = lo if (hi == 0 and lo < body) else body
        st, data = 0, bytes(sr.ham_decode_soft(llr_row[128:128 + 56 * (keep // 7)]))
    elif inner in lrr.ECC:
        st, data = lrr.code_of_ecc(inner).receive(llr_row[128:], body)
    else:
        st, data = fr.decode_stream(llr_row[128:], body, inner - 10)
    if st == 0 and rs:
        out, out_len, fixed = rv.host_row(c.lib, np.frombuffer(data, np.uint8), len(data))
        st, data = (-5, b"") if fixed < 0 else (0, bytes(out[:out_len]))
    if st == 0 and fcs:
        inside = fcs_ref.check(data)
        st, data = (fcs_ref.FRAME_FCS, b"") if inside is None else (0, inside)
    return int(st), (data if st == 0 else b"")


def _whole(want, pay):
    p = pay.cpu().numpy()
    return [f for f, (st, n_out, data) in want.items() if st == 0 and data[:PAYLOAD] == bytes(p[f])]


@pytest.mark.parametrize("ecc", MODES)
def test_chain_is_the_composition_of_the_stages(ecc):
    api = _api()
    c, c0, pay, rx, D = _chain_link(api, ecc, 1400 + ecc)
    assert c.get_llr_weight() == api.LLRW_NOISE
    fe, off, hk, nb, llr, hard = _stages(c, c0, rx, D)
    status = fe["status"].cpu().numpy()
    assert status[EMPTY] == api.FRAME_NOSYNC and (np.delete(status, EMPTY) == 0).all(), status
    q = nb["weight"].cpu().numpy()
    assert (q[EMPTY] == 1).all() and q[TONE].min() < 0.1 and all(q[f].min() > q[TONE].min() for f in range(FRAMES) if f not in (TONE, EMPTY))
    L, H = llr.cpu().numpy(), hard.cpu().numpy()
    body = D * c.bytes_per_symbol - 16
    want = {}
    for f in range(FRAMES):
        if status[f] != 0:
            want[f] = (int(status[f]), 0, b"")
        else:
            st, data = _finish(c, ecc, 0, L[f], H[f], body)
            want[f] = (st, len(data), data)
    r, ones = assert_entry_points_agree(api, c, rx, D)             # decode_batch = decode_host in chunks; every frame alone = decode_long[_host]
    for f, (st, n_out, _, data) in enumerate(ones):
        assert (st, n_out, data) == want[f], f
    c.decode_batch(rx, max_symbols=D)
    trace = c.last_dispatch().split("+")
    assert "k_noise_bins" in trace and "k_sym<llrw>" in trace and "k_sym<llr>" not in trace, trace
    assert trace.index("k_sym<chest>") < trace.index("k_noise_bins") < trace.index("k_sym<llrw>"), trace
    assert_rows_are(r, want)
    assert torch.equal(r["offset"], fe["offset"]) and torch.equal(r["f_delta"], fe["f_delta"]) and torch.equal(r["metric"], fe["metric"])
    good = _whole(want, pay)
    print(f"ecc {ecc}: statuses {[w[0] for w in want.values()]}, {len(good)} of {FRAMES} whole")
    assert len(good) >= FRAMES - 2
    # decode_long and the chunked LLR workspace go through the same kernels
    one = c.decode_long(rx[TONE].contiguous(), D)
    assert "k_noise_bins" in c.last_dispatch() and "k_sym<llrw>" in c.last_dispatch() and one["status"] == want[TONE][0]
    c.set_tuning("soft_chunk_frames", 3)
    assert_rows_are(c.decode_batch(rx, max_symbols=D), want)
    c.set_tuning("soft_chunk_frames", 0)
    # WLS channel estimate and wide CFO acquisition under the mode: the same two kernels behind them
    c2 = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc, chest_mode=api.CHEST_WLS, cfo_mode=api.CFO_WIDE, llr_weight=api.LLRW_NOISE)
    r2 = c2.decode_batch(rx, max_symbols=D)
    t2 = c2.last_dispatch().split("+")
    assert t2.index("k_cfo_wide") < t2.index("k_chest_solve") < t2.index("k_noise_bins") < t2.index("k_sym<llrw>"), t2
    assert int((r2["status"] == 0).sum()) >= FRAMES - 2


@pytest.mark.parametrize("ecc", [12, 16, 94])
def test_combine_chain_is_the_composition_of_the_stages(ecc):
    api = _api()
    R = 2
    c, c0, pay, rx, D = _chain_link(api, ecc, 1500 + ecc, branches=R)
    rows = rx.view(FRAMES * R, -1)
    fe, off, hk, nb, llr, hard = _stages(c, c0, rows, D)
    status = fe["status"].cpu().numpy()
    quality = c.rx_quality(rows, 0, 10, None, off, fe["f_delta"], hk, fe["status"])
    nsym = np.where(status == 0, D, 0).astype(np.int32)              # every capture holds its whole frame
    n_live = (nsym * (c.data_carriers * c.modulation)).astype(np.int32)
    with np.errstate(all="ignore"):
        comb, w = cb.combine(llr.cpu().numpy(), R, quality.cpu().numpy(), status, n_live)
        st_f, nsym_f = cb.merge(R, status, nsym, quality.cpu().numpy())
    want = {}
    for f in range(FRAMES):
        if st_f[f] != 0:
            want[f] = (int(st_f[f]), 0, b"")
        else:
            st, data = _finish(c, ecc, 0, comb[f], None, int(nsym_f[f]) * c.bytes_per_symbol - 16)
            want[f] = (st, len(data), data)
    res = c.decode_combine(rx, max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch().split("+")
    assert "k_llr_combine" in trace and "k_linkq" in trace and "k_sym<llr>" not in trace, trace
    assert trace.index("k_noise_bins") < trace.index("k_sym<llrw>") < trace.index("k_llr_combine"), trace
    assert torch.equal(res["branch_status"].view(-1), fe["status"]) and torch.equal(res["offset"].view(-1), fe["offset"])
    assert torch.equal(res["f_delta"].view(-1), fe["f_delta"]) and torch.equal(res["quality"].view(FRAMES * R, -1), quality)
    assert np.array_equal(res["weight"].view(-1).cpu().numpy(), w)
    assert_rows_are(res, want)
    good = _whole(want, pay)
    print(f"combine ecc {ecc}: statuses {[v[0] for v in want.values()]}, {len(good)} of {FRAMES} whole")
    assert want[EMPTY][0] == api.FRAME_NOSYNC and len(good) >= FRAMES - 2


@pytest.mark.parametrize("ecc", MODES)
def test_mode_off_is_a_context_that_never_heard_of_it(ecc):
    api = _api()
    c, c0, pay, rx, D = _chain_link(api, ecc, 1600 + ecc)
    never = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc)
    c.decode_batch(rx, max_symbols=D)
    assert "k_noise_bins" in c.last_dispatch()
    c.set_llr_weight(api.LLRW_CHANNEL)                              # on, then off again
    off = c.decode_batch(rx, max_symbols=D)
    t_off = c.last_dispatch()
    ref = never.decode_batch(rx, max_symbols=D)
    assert never.last_dispatch() == t_off and "k_noise_bins" not in t_off and "k_sym<llr>" in t_off.split("+")
    assert_same_rows(off, ref)                                      # every key, and the bytes every frame delivered


def test_sc16_decode_under_the_mode_is_the_fc32_decode_of_the_widened_capture():
    api = _api()
    c, c0, pay, rx, D = _chain_link(api, api.ECC_LDPC648, 1650)
    scale = float(2.0 ** -13)
    sc, _ = c.sc16_narrow(rx, 1.0 / scale)
    got = c.decode_batch_sc16(sc, max_symbols=D, scale=scale)
    trace = c.last_dispatch().split("+")
    assert "k_noise_bins" in trace and "k_sym<llrw>" in trace, trace
    assert_same_rows(got, c.decode_batch(c.sc16_widen(sc, scale), max_symbols=D))
    assert int((got["status"] == 0).sum()) >= FRAMES - 2


def test_setter_and_getter_on_a_context():
    api = _api()
    c = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=api.ECC_LDPC648)
    assert c.get_llr_weight() == api.LLRW_CHANNEL == 0
    for bad in (2, -1, 7):
        assert c.lib.ofdm_set_llr_weight(c.h, bad) == -1 and c.get_llr_weight() == 0
    c.set_llr_weight(api.LLRW_NOISE)
    assert c.get_llr_weight() == 1 and c.lib.ofdm_set_llr_weight(c.h, 2) == -1 and c.get_llr_weight() == 1
    with pytest.raises(api.OfdmError):
        c.set_llr_weight(2)
    assert c.lib.ofdm_get_llr_weight(c.h, None) == -1
    assert api.Context(n_fft=N, llr_weight=api.LLRW_NOISE).get_llr_weight() == 1


@pytest.mark.parametrize("ecc", [0, 1, 20, 64, 65, 84])
def test_modes_without_llrs_do_not_change(ecc):
    api = _api()
    c = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc)
    pay, rx = link_on(c, FRAMES, PAYLOAD, 25.0, 1700 + ecc)
    D = c.data_symbols(PAYLOAD)
    a = c.decode_batch(rx, max_symbols=D)
    t_a = c.last_dispatch()
    c.set_llr_weight(api.LLRW_NOISE)
    b = c.decode_batch(rx, max_symbols=D)
    assert c.last_dispatch() == t_a and "k_noise_bins" not in t_a and "llr" not in t_a, t_a
    assert "k_rxframe64" in t_a                                      # the fused frame kernel still runs
    assert_same_rows(a, b)                                          # every key, and the bytes every frame delivered
    assert int((a["status"] == 0).sum()) >= FRAMES - 1


# ---------------------------------------------------------------------------------------------------------- 5. one link
def test_one_link_with_a_tone(orc):
    """The CPU test's link (N = 64, 64-QAM, guard bands, LDPC648, 560-byte payloads, 14 dB, a tone 10 dB under the frame at bin 11.3), 64
    frames through decode_batch: the mode on delivers at least 48 whole, off at most 16, and neither delivers a wrong frame.
    Measured: on 61 / 64, off 0 / 64."""
    api = _api()
    payload, frames = 560, 64
    rng = np.random.default_rng(1800)
    pays = rng.integers(0, 256, (frames, payload), dtype=np.uint8)
    caps = np.stack([fc32(nw.tone_capture(orc, ldpc_ref.stream(bytes(pays[f])), 14.0, 1800 + f, -10.0)) for f in range(frames)])
    count = {}
    for mode in (api.LLRW_CHANNEL, api.LLRW_NOISE):
        c = api.Context(n_fft=64, modulation=6, guard_bands=True, ecc=api.ECC_LDPC648, llr_weight=mode)
        D = c.data_symbols(payload)
        r = c.decode_batch(c.to_device(caps), max_symbols=D)
        c.synchronize()
        st, ln, by = r["status"].cpu().numpy(), r["len"].cpu().numpy(), r["bytes"].cpu().numpy()
        right = [f for f in range(frames) if st[f] == 0 and ln[f] == payload and bytes(by[f, :payload]) == bytes(pays[f])]
        wrong = [f for f in range(frames) if st[f] == 0 and f not in right]
        print(f"llr_weight {mode}: {len(right)} right, {len(wrong)} wrong, {frames - len(right) - len(wrong)} reported, of {frames}")
        assert not wrong, (mode, wrong)
        count[mode] = len(right)
    assert count[api.LLRW_NOISE] >= 48 and count[api.LLRW_CHANNEL] <= 16, count
