"""Every kernel and host table that reads a pilot table, against its definition UNDER A TABLE OTHER THAN THE DEFAULT (the families of
tests/pilot_cases.py, certified on the CPU by tests/test_pilots_cpu.py): the preamble and the training table are inputs of a context,
and a link against the reference's own transmitter, or any other radio, runs every kernel with tables the rest of the suite never
builds.  Every test names the kernel it is meant for by last_dispatch().  The references take the table as an argument and are the
suite's own: orc.encode / decode_sc / estimate_channel / rx_demod, chest_ref, quality_ref, cfo_wide_ref, soft_ref, packets_ref, the
compositions of chain_refs and of the mode tests; the bars are those of the tests that hold the same kernels under the default table.

A zero training bin (`holes`): under CHEST_LS the estimate is NaN in that bin on both sides, a data carrier there demaps by the NaN
rule (all bits 0) and -- w_k being a mean over all data carriers -- every LLR of the frame is 0; so the soft chains run `holes` under
CHEST_WLS, where the bin weighs 0 and H' is finite (include/ofdm_hip.h at ofdm_create)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_refs  # noqa: E402
import chest_ref as cr  # noqa: E402
import framed_ref as fr  # noqa: E402
import ldpc_ref  # noqa: E402
import packets_ref as P  # noqa: E402
import pilot_cases as pc  # noqa: E402
import quality_ref as qr  # noqa: E402
import soft_ref as sr  # noqa: E402
import test_gpu_cfo_wide as tcw  # noqa: E402
import test_gpu_chest as tch  # noqa: E402
import test_gpu_combine as tcb  # noqa: E402
import test_gpu_llr_oracle as tlo  # noqa: E402
import test_gpu_quality as tq  # noqa: E402
from chain_checks import assert_entry_points_agree, assert_rows_are, assert_same_rows, ofdm_api as _api  # noqa: E402
from tools.link import link, wide_link_on  # noqa: E402
from util import assert_bytes_match, loud_payload, rel_err, through_channel, wide  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
FAMILIES = pc.FAMILIES


def _ctx(api, name, n, mod, guard, **kw):
    pre, trn = pc.tables(name, n)
    return api.Context(n_fft=n, modulation=mod, guard_bands=guard, preamble=pre, training=trn, **kw)


def _tables_kw(name, n):
    pre, trn = pc.tables(name, n)
    return dict(preamble=pre, training=trn)


def _chest_for(api, name):
    """the channel-estimate mode a family's SOFT chains run under (module docstring)"""
    return api.CHEST_WLS if name == "holes" else api.CHEST_LS


@functools.lru_cache(maxsize=None)
def _data_mask(n, guard):
    from oracle import oracle as orc

    return np.array([orc.carrier_class(i, n, bool(guard)) == 0 for i in range(n)])


def _i32(c, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(c.device)


def _f64(c, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(c.device)


# ---------------------------------------------------------------------------------------------------------- 1. transmit
def _assert_frames_are_the_oracle(orc, frames, pay, lens, name, n, mod, guard):
    """frames (host, complex64 [F, slot]) against orc.encode under the family's tables: the suite's 1e-5 norm-relative per frame, the four
    preamble copies bit-identical, the signed maximum 1 within 1e-6 -> the oracle's frames"""
    S = n + n // 4
    pre, trn = pc.tables(name, n)
    want = [orc.encode(bytes(pay[f, :lens[f]]), guard, mod, n, preamble=pre, training=trn) for f in range(len(pay))]
    for f, w in enumerate(want):
        got = frames[f]
        assert rel_err(got[:w.size], w) <= TOL, (name, n, f, int(lens[f]), rel_err(got[:w.size], w))
        for r in (2, 3, 4):
            assert np.array_equal(got[S:2 * S].view(np.uint64), got[r * S:(r + 1) * S].view(np.uint64)), (name, n, f, r)
        assert abs(max(got.real.max(), got.imag.max()) - 1.0) < 1e-6, (name, n, f)
        assert not np.any(got[w.size:].real > 1.0) and np.isfinite(got).all()
    return want


TX_SHAPES = [  # n_fft, modulation, guard, payload bytes, frames, tuning, dispatch
    (64, 6, True, 560, 8, {}, "k_txframe64"),
    (256, 4, True, 300, 5, {}, "k_txframe_mid"),
    (512, 4, True, 3 * 192 - 16, 5, {}, "k_txframe_mid<once>"),     # data symbols within one workgroup step: built once (N >= 512)
    (4096, 2, False, 2 * 1024 - 16, 2, {}, "k_txframe4096"),
]


@pytest.mark.parametrize("n,mod,guard,nbytes,nfr,tuning,want_kernel", TX_SHAPES, ids=[s[-1] for s in TX_SHAPES])
@pytest.mark.parametrize("name", FAMILIES)
def test_transmit_under_the_table(orc, name, n, mod, guard, nbytes, nfr, tuning, want_kernel):
    api = _api()
    rng = np.random.default_rng([n, mod, nbytes, 1])
    lens = rng.integers(0, nbytes + 1, nfr).astype(np.int32)
    lens[0], lens[-1] = nbytes, 0                                       # ragged, 0 .. nbytes
    pay = rng.integers(0, 256, (nfr, nbytes), dtype=np.uint8)
    c = _ctx(api, name, n, mod, guard, tuning=tuning)
    frames = c.encode_batch(c.to_device(pay), lens=torch.from_numpy(lens))
    assert c.last_dispatch() == want_kernel, c.last_dispatch()
    _assert_frames_are_the_oracle(orc, frames.cpu().numpy(), pay, lens, name, n, mod, guard)
    # other tables, other frames: the default context's header is not this one's
    base = api.Context(n_fft=n, modulation=mod, guard_bands=guard).encode_batch(c.to_device(pay), lens=torch.from_numpy(lens))
    assert rel_err(frames[0].cpu().numpy(), base[0].cpu().numpy()) > 1e-3


def test_unit_loud_quiet_and_loud_frame(orc):
    """The maximum every transmit kernel starts from is the header's SIGNED maximum over re and im.  Under unit_loud that is 0.95, the
    imaginary part of a preamble sample, next to a real part of -0.99.  A quiet frame (its data symbols peak far below) keeps its
    maximum there, and its most negative component is -0.99 / 0.95 < -1; a util.loud_payload frame, N = 64 without guard bands, is
    louder than its header and is scaled by its own data symbol."""
    api = _api()
    n, mod, S = 64, 6, 80
    nbytes = 2 * 48 - 16
    neg, pos = pc.loud_positions(n)
    rng = np.random.default_rng(95)
    pay = np.stack([rng.integers(0, 256, nbytes, dtype=np.uint8), loud_payload(orc, n, mod, nbytes, 1, seed=3)])
    lens = np.array([nbytes, nbytes], np.int32)
    c = _ctx(api, "unit_loud", n, mod, False)
    frames = c.encode_batch(c.to_device(pay)).cpu().numpy()
    assert c.last_dispatch() == "k_txframe64"
    want = _assert_frames_are_the_oracle(orc, frames, pay, lens, "unit_loud", n, mod, False)
    value, at, part = pc.signed_peak(frames[0])
    assert (at, part) == (S + pos, "im") and pc.signed_peak(want[0])[1:] == (at, part)
    assert abs(frames[0][S + pos].imag - 1.0) < 1e-6 and abs(frames[0][S + neg].real + 0.99 / 0.95) < 1e-6
    assert frames[0].real.min() == frames[0][S + neg].real < -1.0         # abs would have scaled this frame by 1 / 0.99
    value, at, part = pc.signed_peak(frames[1])
    assert at >= 10 * S and pc.signed_peak(want[1])[1:] == (at, part)     # the loud frame peaks in a data symbol
    hdr_peak = pc.signed_peak(frames[1][:10 * S])
    assert hdr_peak[1:] == (S + pos, "im") and hdr_peak[0] < 0.9, hdr_peak  # ... louder than 0.95 before normalisation
    print(f"quiet frame: minimum {frames[0].real.min():.4f}; loud frame: header peak {hdr_peak[0]:.4f} after scaling")


@pytest.mark.parametrize("name", FAMILIES)
def test_fused_sc16_transmit_under_the_table(name):
    """rows and clipped counts of encode_batch_sc16 at scale 32767 are ofdm_sc16_narrow of encode_batch's rows, bit for bit; under
    unit_loud a quiet frame's -0.99 / 0.95 lies below -1, so its count is not 0"""
    api = _api()
    rng = np.random.default_rng(1600)
    pay = rng.integers(0, 256, (5, 200), dtype=np.uint8)
    c = _ctx(api, name, 64, api.QAM64, True)
    fc = c.encode_batch(c.to_device(pay)).cpu().numpy()
    assert c.last_dispatch() == "k_txframe64"
    got, clipped = c.encode_batch_sc16(c.to_device(pay), 32767.0, want_clipped=True)
    assert c.last_dispatch() == "k_txframe64_sc16"
    got, clipped = got.cpu().numpy(), clipped.cpu().numpy()
    for f in range(pay.shape[0]):
        want, n_clipped = api.sc16_narrow(fc[f], 32767.0)
        assert np.array_equal(got[f], want), (name, f)
        assert int(clipped[f]) == n_clipped, (name, f, int(clipped[f]), n_clipped)
        assert (n_clipped > 0) == (name == "unit_loud"), (name, f, n_clipped)
    print(f"{name}: clipped components per frame {clipped.tolist()}")


# ---------------------------------------------------------------------------------------------------------- 2. receive, hard decisions
def _assert_decode_is_the_oracle(r, k, mod, what):
    """decode_batch's result against orc.decode_sc(..., training=) of the same captures: status and offset equal, f_delta within 1e-9,
    bytes under util.assert_bytes_match with the oracle's soft points (stream bit b of the body is bit 128 + b) -> excused points"""
    st, off, fd, ln, by = (r[x].cpu().numpy() for x in ("status", "offset", "f_delta", "len", "bytes"))
    head = bytes(16)
    excused = 0
    for f, w in enumerate(k["want"]):
        assert w["status"] == 0 and st[f] == 0, (what, f, int(st[f]), w["status"])
        assert off[f] == w["offset"] and abs(fd[f] - w["f_delta"]) <= 1e-9, (what, f, int(off[f]), w["offset"], float(fd[f]), w["f_delta"])
        assert ln[f] == len(w["bytes"]), (what, f, int(ln[f]), len(w["bytes"]))
        excused += assert_bytes_match(head + bytes(by[f, :ln[f]]), head + w["bytes"], w["soft"], mod, what=f"{what} frame {f}")
    return excused


RX_PATHS = [  # n_fft, modulation, guard, payload bytes, tuning, the kernels the chain must name
    (64, 6, True, 560, {}, ("k_rxframe64<finish>",)),
    (1024, 4, True, 1000, {}, ("k_rxframe1024<finish>",)),
    (256, 2, False, 300, {"no_mid_kernels": 1}, ("k_sym<chest>", "k_sym<demod>", "k_rx_finish")),           # the generic pair
]


@pytest.mark.parametrize("n,mod,guard,nbytes,tuning,kernels", RX_PATHS, ids=[p[-1][0] for p in RX_PATHS])
@pytest.mark.parametrize("name", FAMILIES)
def test_decode_under_the_table(name, n, mod, guard, nbytes, tuning, kernels):
    """decode_batch with ECC_NONE on six captures of the family (30 dB, a delay below S, a CFO inside +-0.9 pi / S) through the fused
    frame kernels and the generic pair, against orc.decode_sc(..., training=): status, offset, f_delta to 1e-9, bytes under the
    unchanged 1e-5 rule (the number of excused points is printed; 0 is expected).  Under `holes` the dead data carriers' points are
    NaN in the oracle, and the decisions there are the NaN rule's on both sides: all bits 0, so no payload comes back whole."""
    api = _api()
    k = pc.rx_hard_case(name, n, mod, guard, nbytes)
    c = _ctx(api, name, n, mod, guard, tuning=tuning)
    assert k["D"] == c.data_symbols(nbytes) and (n < 1024 or k["D"] <= 6)
    r = c.decode_batch(c.to_device(k["rx"]), max_symbols=k["D"])
    c.synchronize()
    trace = c.last_dispatch().split("+")
    assert all(x in trace for x in kernels) and ("rxframe" in c.last_dispatch()) == (not tuning), trace
    excused = _assert_decode_is_the_oracle(r, k, mod, (name, n))
    pay_ok = sum(bytes(r["bytes"][f, :nbytes].cpu().numpy()) == bytes(k["pay"][f]) for f in range(len(k["want"])))
    dead = pc.dead_bins(k["trn"])
    print(f"{name} N {n}: {excused} excused points, {pay_ok} of {len(k['want'])} payloads whole, {dead.size} dead bins")
    dead_data = int(_data_mask(n, guard)[dead].sum())
    assert (dead_data > 0) == (name == "holes")
    for w in k["want"]:
        assert np.isnan(np.asarray(w["soft"]).real).sum() == k["D"] * dead_data


@pytest.mark.parametrize("n,mod,guard,nbytes", [(64, 6, True, 560), (256, 2, False, 300)])
@pytest.mark.parametrize("name", FAMILIES)
def test_channel_estimate_and_generic_demod_under_the_table(orc, name, n, mod, guard, nbytes):
    """ofdm_estimate_channel_batch (k_sym<chest>, which reads 1 / t_k) against orc.estimate_channel with the family's table: 1e-5
    norm-relative over the live bins, non-finite in exactly the dead bins on both sides; then the generic demodulator with that
    estimate (k_sym<demod>: decode_batch has no key that turns k_rxframe64 off, so the N = 64 generic pair runs through its stage
    entry points) against orc.rx_demod given the device's estimate -- the NaN rule included."""
    api = _api()
    k = pc.rx_hard_case(name, n, mod, guard, nbytes)
    S, D, trn = n + n // 4, k["D"], k["trn"]
    c = _ctx(api, name, n, mod, guard, tuning={"no_fast64": 1, "no_mid_kernels": 1})
    rx = c.to_device(k["rx"])
    off, fd = _i32(c, [w["offset"] for w in k["want"]]), _f64(c, [w["f_delta"] for w in k["want"]])
    hk = c.estimate_channel(rx, off, fd)
    assert c.last_dispatch() == "k_sym<chest>"
    hard = c.rx_demod(rx, D, first_symbol=10, offset=off, f_delta=fd, hk=hk)
    assert c.last_dispatch() == "k_sym<demod>"
    c.synchronize()
    hk, hard = hk.cpu().numpy(), hard.cpu().numpy()
    live = trn != 0
    excused, worst = 0, 0.0
    for f, w in enumerate(k["want"]):
        rot = orc.cfo_rotate(wide(k["rx"][f])[w["offset"]:w["offset"] + (10 + D) * S], w["f_delta"], 0)
        with np.errstate(all="ignore"):
            want = orc.estimate_channel(rot[5 * S:10 * S], trn, n)
            ob, soft = orc.rx_demod(rot[10 * S:], n, guard, mod, hk=wide(hk[f]), want_soft=True)
        assert np.array_equal(np.isfinite(want), live) and np.array_equal(np.isfinite(hk[f]), live), (name, f)
        worst = max(worst, rel_err(hk[f][live], want[live]))
        excused += assert_bytes_match(bytes(hard[f]), ob, soft, mod, what=f"{name} N {n} frame {f}")
        assert np.isnan(np.asarray(soft).real).sum() == D * int((~live & _data_mask(n, guard)).sum())
    print(f"{name} N {n}: LS estimate {worst:.2e} of the oracle's over the live bins, {excused} excused points")
    assert worst <= TOL


# ---------------------------------------------------------------------------------------------------------- 3. receive, soft
@pytest.mark.parametrize("n,mod,nbytes", [(64, 6, 560), (256, 4, 600)])
@pytest.mark.parametrize("name", FAMILIES)
def test_llrs_under_the_table(orc, name, n, mod, nbytes):
    """rx_llr (k_sym<llr>) as the decode chain calls it, with the device's own estimate under the family's table (held to the oracle
    above), against soft_ref.oracle_llr_reference given the same estimate, by the rule of tests/test_gpu_llr_oracle.py.  Under `holes`
    the LS estimate is NaN on dead data carriers and every LLR of the frame is 0 on both sides; the denoised H' is finite."""
    api = _api()
    k = pc.rx_hard_case(name, n, mod, True, nbytes)
    S, D = n + n // 4, k["D"]
    c = _ctx(api, name, n, mod, True)
    rx = c.to_device(k["rx"])
    off, fd = _i32(c, [w["offset"] for w in k["want"]]), _f64(c, [w["f_delta"] for w in k["want"]])
    ls = c.estimate_channel(rx, off, fd)
    X = np.stack([orc.cfo_rotate(wide(k["rx"][f])[w["offset"]:w["offset"] + (10 + D) * S], w["f_delta"], 0)[10 * S:] for f, w in enumerate(k["want"])])
    for label, hk in [("LS", ls)] + ([("WLS", c.chest_smooth(ls))] if name == "holes" else []):
        got = c.rx_llr(rx, D, first_symbol=10, offset=off, f_delta=fd, hk=hk)
        assert c.last_dispatch() == "k_sym<llr>"
        c.synchronize()
        got = got.cpu().numpy()
        ref = sr.oracle_llr_reference(orc, X, n, True, mod, tlo.SCALE, hk.cpu().numpy())
        tlo._hold(got, ref, f"{name} N {n} {label}")
        if name == "holes" and label == "LS":
            assert not np.isfinite(ref["y"]).any() and not got.any()
        else:
            assert np.isfinite(ref["y"]).all() and (got != 0).mean() > 0.9


SOFT_CHAINS = [("ECC_LDPC648", 0), ("ECC_CONV_K7F_R34", 0), ("ECC_LDPC648", 1)]


@pytest.mark.parametrize("ecc_name,noise_weight", SOFT_CHAINS, ids=["ldpc648", "conv_k7f_r34", "ldpc648-llrw_noise"])
@pytest.mark.parametrize("name", FAMILIES)
def test_soft_chain_is_the_composition_of_the_stages(name, ecc_name, noise_weight):
    """decode_batch of a soft mode on the seeded link of tools/link.py built with the family's tables: bit for bit the stages composed
    by hand (chain_refs; under LLRW_NOISE noise_bins and the weighted LLRs, k_noise_bins + k_sym<llrw>), and the payloads at 30 dB"""
    api = _api()
    ecc = getattr(api, ecc_name)
    n, F, payload = 64, 5, 300
    c, pay, rx, D = link(ecc, n, api.QAM16, F, payload, 30.0, 70 + ecc + noise_weight, chest_mode=_chest_for(api, name),
                         llr_weight=noise_weight, **_tables_kw(name, n))
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch().split("+")
    assert "k_sym<chest>" in trace and ("k_chest_solve" in trace) == (name == "holes"), trace
    assert ("k_noise_bins" in trace and "k_sym<llrw>" in trace and "k_sym<llr>" not in trace) if noise_weight else ("k_sym<llr>" in trace), trace
    assert (r["status"] == 0).all(), r["status"].tolist()
    if noise_weight:
        hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
        nb = c.noise_bins(rx, r["offset"], r["f_delta"], r["status"])
        assert c.last_dispatch() == "k_noise_bins"
        L = c.rx_llr(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk, bin_weight=nb["weight"])
        assert c.last_dispatch() == "k_sym<llrw>"
        c.synchronize()
        L = L.cpu().numpy()
    else:
        _, L = chain_refs.hard_and_llrs(c, rx, r, D)
    body = D * c.bytes_per_symbol - 16
    want = {}
    for f in range(F):
        st, data = ldpc_ref.receive(L[f, 128:], body) if ecc == api.ECC_LDPC648 else fr.decode_stream(L[f, 128:128 + 8 * body], body, 2)
        want[f] = (st, len(data), data)
    assert_rows_are(r, want)
    p = pay.cpu().numpy()
    assert all(st == 0 and bytes(data[:payload]) == bytes(p[f]) for f, (st, _, data) in want.items())


# ---------------------------------------------------------------------------------------------------------- 4. the denoised estimate
@pytest.mark.parametrize("n_frames", [1, 3, pc.CHEST_ROWS])
@pytest.mark.parametrize("n_fft", [64, 128, 1024, 4096])
@pytest.mark.parametrize("name", ["unit_loud", "holes"])
def test_chest_stage_under_the_table(name, n_fft, n_frames):
    """tests/test_gpu_chest.py's stage test with W_k = |t_k|^2 and R^-1 of the family's table; under `holes` the rows are NaN in the
    dead bins, as LS leaves them, and the output is finite in every bin: k_chest_weight's wk == 0 branch"""
    api = _api()
    rows, want, measured, tol = pc.chest_stage_case(name, n_fft)
    ROWS = pc.CHEST_ROWS
    pick = {1: [ROWS - 2], 3: [0, 1, ROWS - 1]}.get(n_frames, list(range(ROWS)))
    dead = pc.dead_bins(pc.tables(name, n_fft)[1])
    assert np.array_equal(np.nonzero(~np.isfinite(rows[0]))[0], dead) and np.isfinite(rows[ROWS - 1]).all() and np.isfinite(want).all()
    c = _ctx(api, name, n_fft, api.BPSK, False)
    x = c.to_device(rows[pick])
    got = c.chest_smooth(x)
    c.synchronize()
    assert "k_chest_solve" in c.last_dispatch() and c.last_dispatch().startswith("k_chest_weight")
    g = got.cpu().numpy()
    assert np.isfinite(g).all()                                       # dead bins included
    err = max(rel_err(g[i], want[r]) for i, r in enumerate(pick))
    print(f"{name} n_fft {n_fft}, {n_frames} rows: complex64 restatement {measured:.2e}, kernel {err:.2e}, allowed {tol:.2e}")
    assert err <= tol
    for cap in (1, 3):
        c.set_tuning("grid_cap", cap)
        assert torch.equal(c.chest_smooth(x), got), cap
    c.set_tuning("grid_cap", 0)
    y = x.clone()
    assert c.chest_smooth(y, out=y) is y and torch.equal(y, got)
    # the default table's weights and matrix give another answer: the context's own tables were read
    other = api.Context(n_fft=n_fft).chest_smooth(torch.nan_to_num(x))
    assert max(rel_err(other.cpu().numpy()[i], want[r]) for i, r in enumerate(pick)) > 10 * tol


def test_a_band_nulled_table_is_refused_by_the_wls_mode_not_by_the_others():
    """A training table that is zero on the whole guard band (tests/test_pilots_cpu.py: cond(R) 2e14 at N = 256, where the host solve
    used to return rounding residue): a context that asks for CHEST_WLS is refused and so is the stage; LS contexts work as ever.  At
    N = 64 (cond 7e2) R^-1 is a true inverse and the mode is served."""
    api = _api()
    x = np.ones((2, 256), np.complex64)
    trn = pc.band_nulled(256)
    with pytest.raises(api.OfdmError):
        api.Context(n_fft=256, training=trn, chest_mode=api.CHEST_WLS)
    ls = api.Context(n_fft=256, training=trn)
    xd = ls.to_device(x)
    assert ls.lib.ofdm_chest_smooth_batch(ls.h, xd.data_ptr(), 2, xd.data_ptr()) == -1
    assert ls.fft(xd).shape == xd.shape                                # (the context itself is fine)
    t64, one = pc.band_nulled(64), np.ones((1, 64), np.complex64)
    ok = api.Context(n_fft=64, training=t64, chest_mode=api.CHEST_WLS)
    got = ok.chest_smooth(ok.to_device(one)).cpu().numpy()
    want = cr.smooth(wide(one), t64, 64)                               # (H = 1 is one tap inside the window: kept, 6e-14 in f64)
    measured = rel_err(cr.smooth_c64(one, t64, 64), want)
    err = rel_err(got, want)
    print(f"band-nulled N 64: complex64 restatement {measured:.2e}, kernel {err:.2e}")
    assert "k_chest_solve" in ok.last_dispatch() and rel_err(want, one) < 1e-12 and err <= max(4.0 * measured, 1e-5)


@pytest.mark.parametrize("ecc_name", ["ECC_NONE", "ECC_CONV_K7F_R34"])
@pytest.mark.parametrize("n", [64, 1024])
def test_wls_chain_under_holes_is_the_composition_of_the_stages(orc, n, ecc_name):
    """tests/test_gpu_chest.py's test_chain_with_the_mode_is_the_composition_of_the_stages under `holes`"""
    api = _api()
    ecc = getattr(api, ecc_name)
    mod = api.QPSK if n == 1024 else api.QAM16
    c, pay, rx, D = link(ecc, n, mod, 5, 300, 30.0, 40 + n, chest_mode=api.CHEST_WLS, **_tables_kw("holes", n))
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    assert "k_chest_weight" in c.last_dispatch() and "k_chest_solve" in c.last_dispatch() and "k_rxframe" not in c.last_dispatch()
    d, fd, _ = c.sc_correlate(rx)
    assert torch.equal(r["offset"], torch.clamp(d - c.S - 4, min=0).to(torch.int32)) and torch.equal(r["f_delta"], fd)
    want = tch._staged_reference(c, rx, r, D, ecc, orc)
    assert len(want) == 5 and all(st == 0 for st, _, _ in want.values())
    assert_rows_are(r, want)
    good = [f for f, (st, n_out, data) in want.items() if bytes(data[:300]) == bytes(pay[f].cpu().numpy())]
    print(f"holes N {n} {ecc_name}: {len(good)} of 5 payloads whole")
    assert len(good) >= (5 if ecc != api.ECC_NONE else 3)
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    assert bool(torch.isfinite(torch.view_as_real(hk)).all())
    if ecc == api.ECC_NONE:                                           # the hard bytes are the oracle's, given the device's H', offset and CFO
        hard = c.rx_demod(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
        c.synchronize()
        S = c.S
        for f in range(rx.shape[0]):
            x = np.concatenate([wide(rx[f].cpu().numpy()), np.zeros((10 + D) * S, np.complex128)])
            o = int(r["offset"][f])
            rot = orc.cfo_rotate(x[o:o + (10 + D) * S], float(r["f_delta"][f]), 0)
            ob, soft = orc.rx_demod(rot[10 * S:], n, True, mod, hk=wide(hk[f].cpu().numpy()), want_soft=True)
            assert_bytes_match(bytes(hard[f].cpu().numpy()), ob, soft, mod, what=f"frame {f}")


# ---------------------------------------------------------------------------------------------------------- 5. link quality
@functools.lru_cache(maxsize=None)
def _quality_case(name, n):
    """tests/test_gpu_quality.py's kernel case under a family's tables: six frames through the FIR channel with a delay and a CFO each
    (odd row stride), a per-frame estimate -- the oracle's LS estimate, under `holes` its denoised form (finite in the dead bins) --
    and the reference rows with sum |t_k|^2 of the family's table"""
    from oracle import oracle as orc

    orc.lib()
    mod, guard, frames, D = (6, True, 6, 4) if n == 64 else (4, True, 6, 3)
    S, nd = n + n // 4, orc.data_carriers(n, guard)
    pre, trn = pc.tables(name, n)
    payload = D * nd * mod // 8 - 16 - 3
    n_points = -(-8 * (16 + payload) // mod)
    span = (10 + D) * S + 2 * n // 4 + 61
    span += 1 - span % 2
    for seed in range(8):
        rng = np.random.default_rng([n, mod, FAMILIES.index(name), seed])
        rx = np.zeros((frames, span), np.complex64)
        off = rng.integers(0, n // 4, frames).astype(np.int32)
        fd = (rng.random(frames) - 0.5) * 2.0 / S
        for f in range(frames):
            tx = orc.encode(bytes(rng.integers(0, 256, payload, dtype=np.uint8)), guard, mod, n, preamble=pre, training=trn)
            rx[f] = through_channel(orc, rng, tx, span, int(off[f]), float(fd[f]), tq.SNR[mod], data_start=10 * S)
        fd = fd + rng.standard_normal(frames) * 1e-3 / S
        rows = []
        with np.errstate(all="ignore"):
            for f in range(frames):
                x = orc.cfo_rotate(wide(rx[f, off[f]:off[f] + 10 * S]), float(fd[f]), 0)
                rows.append(orc.estimate_channel(x[5 * S:], trn, n))
        hk = np.asarray(rows)
        if name == "holes":
            hk = cr.smooth(hk, trn, n)
        hk = hk.astype(np.complex64)
        ref = tq._reference(rx, n, guard, mod, trn, D, n_points, offset=off, f_delta=fd, hk=hk)
        if float(np.mean(ref[2] > 0)) == 0.0:
            break
    assert float(np.mean(ref[2] > 0)) == 0.0
    return dict(rx=rx, off=off, fd=fd, hk=hk, n_points=n_points, ref=ref, mod=mod, guard=guard, D=D, trn=trn)


@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("name", FAMILIES)
def test_link_quality_under_the_table(name, n):
    """rx_quality (k_linkq) against quality_ref.quality(..., training=the family's table, ...) with the bars of
    tests/test_gpu_quality.py::test_kernel_matches_the_definition; gain, snr and llr_unit are the fields that read sum |t_k|^2 over the
    data carriers (a dead data bin adds 0 to it)"""
    api = _api()
    k = _quality_case(name, n)
    want, tol, near, widen, dist = k["ref"]
    assert np.all(want[:, qr.Q_VALID] == 1) and np.all(want[:, qr.Q_POINTS] == k["n_points"]) and np.isfinite(want).all()
    c = _ctx(api, name, n, k["mod"], k["guard"])
    got = c.rx_quality(c.to_device(k["rx"]), k["D"], n_points=k["n_points"], offset=_i32(c, k["off"]), f_delta=_f64(c, k["fd"]),
                       hk=c.to_device(k["hk"]))
    c.synchronize()
    assert c.last_dispatch() == "k_linkq"
    worst = tq._assert_rows(got.cpu().numpy(), want, tol, near, widen, (name, n))
    # the default table's sum would have been another: the gain field tells the two apart by far more than its tolerance
    data = _data_mask(n, True)
    t2, t2_default = float(np.sum(np.abs(k["trn"][data]) ** 2)), float(np.sum(np.abs(pc.tables("default", n)[1][data]) ** 2))
    assert abs(t2 / t2_default - 1.0) > 10 * tol[qr.Q_GAIN], (t2, t2_default)
    print(f"{name} N {n}: restatement {({qr.NAMES[f]: f'{v:.1e}' for f, v in dist.items()})}, kernel {({a: f'{v:.1e}' for a, v in worst.items()})}, "
          f"sum |t|^2 {t2:.2f} (default {t2_default:.2f})")


# ---------------------------------------------------------------------------------------------------------- 6. wide CFO acquisition
@pytest.mark.parametrize("n", sorted(pc.WIDE_SNR))
@pytest.mark.parametrize("name", FAMILIES)
def test_cfo_wide_under_the_table(name, n):
    """cfo_wide (k_cfo_wide, matched against conj(t) of the context's table) against cfo_wide_ref.cfo_wide(x, n, the family's table, ...):
    m exact -- tests/test_pilots_cpu.py holds the true m to a best-to-runner-up ratio of 2 on these captures under every family --,
    f_delta bit for bit, the metrics within the bar of tests/test_gpu_cfo_wide.py"""
    api = _api()
    k = pc.cfo_wide_case(name, n)
    m, fd, g = k["ref"]
    assert np.array_equal(m, k["m"]) and (g[:, 0] / g[:, 1]).min() >= 2.0
    c = _ctx(api, name, n, 6, True)
    rx, off, f0 = c.to_device(k["rx"]), _i32(c, k["off"]), _f64(c, k["f0"])
    r = c.cfo_wide(rx, off, f0, 8)
    c.synchronize()
    assert c.last_dispatch() == "k_cfo_wide"
    worst = tcw._assert_rows(r, m, fd, g, k["tol"], (name, n))
    print(f"{name} N {n}: ratio min {(g[:, 0] / g[:, 1]).min():.2f}, restatement {k['dist']:.1e}, kernel {worst:.1e}, tol {k['tol']:.1e}")
    # the default table matched against these frames is another metric altogether
    d = api.Context(n_fft=n, modulation=6, guard_bands=True).cfo_wide(rx, off, f0, 8)
    assert not torch.allclose(d["metric"], r["metric"], rtol=0.05)


@pytest.mark.parametrize("name", FAMILIES)
def test_wide_cfo_chain_delivers_the_payload_at_m_5(name):
    api = _api()
    n, F, payload = 64, 3, 120
    c = _ctx(api, name, n, api.QPSK, True, cfo_mode=api.CFO_WIDE, chest_mode=_chest_for(api, name))
    m = torch.full((F,), 5, dtype=torch.int32, device=c.device)
    pay, rx, m, fd = wide_link_on(c, F, payload, 30.0, 5005, m=m)
    D = c.data_symbols(payload)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    assert "k_cfo_wide" in c.last_dispatch().split("+"), c.last_dispatch()
    assert (r["status"] == 0).all() and (r["len"] == payload).all()
    assert torch.equal(r["bytes"][:, :payload], pay)
    err = (r["f_delta"] - fd).abs().max().item()
    assert err <= 0.05 * 2.0 * np.pi / c.S, err                       # the channel's own offset, modulo nothing


# ---------------------------------------------------------------------------------------------------------- 7. the other entry points
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("name", ["stdrng", "holes"])
def test_every_decode_entry_point_under_the_table(name, soft):
    """decode_batch = decode_host in chunks = every frame alone through decode_batch, decode_long, decode_long_host and api.decode (the
    free function, handed the tables), and the sc16 forms = the fc32 forms of the widened capture"""
    api = _api()
    n, mod, F, payload = 64, api.QAM16, 5, 300
    ecc = api.ECC_CONV_K7F_R34 if soft else api.ECC_NONE
    kw = dict(_tables_kw(name, n), chest_mode=_chest_for(api, name) if soft else api.CHEST_LS)
    c, pay, rx, D = link(ecc, n, mod, F, payload, 30.0, 300 + soft, **kw)
    r, ones = assert_entry_points_agree(api, c, rx, D, decode_kw=dict(ecc=ecc, **kw))
    assert ("k_rxframe64" in c.last_dispatch()) == (not soft)
    assert (r["status"] == 0).all()
    if soft:
        assert all(n_out == payload and data == bytes(pay[f].cpu().numpy()) for f, (st, n_out, off, data) in enumerate(ones))
    scale = float(2.0 ** -13)
    sc, _ = c.sc16_narrow(rx, 1.0 / scale)
    widened = c.sc16_widen(sc, scale)
    ref = c.decode_batch(widened, max_symbols=D)
    c.synchronize()
    assert_same_rows(c.decode_batch_sc16(sc, max_symbols=D, scale=scale), ref)
    assert_same_rows(c.decode_host_sc16(sc.cpu().numpy(), max_symbols=D, scale=scale), ref)
    one = c.decode_long_sc16(sc[1].contiguous(), D, scale=scale)
    assert (one["status"], one["len"], one["offset"]) == (int(ref["status"][1]), int(ref["len"][1]), int(ref["offset"][1]))
    assert torch.equal(one["bytes"][: one["len"]], ref["bytes"][1, : one["len"]])


@pytest.mark.parametrize("name", ["stdrng", "holes"])
def test_packets_laid_back_to_back_under_the_table(orc, name):
    api = _api()
    n, mod, nbytes = 64, api.QAM16, 200
    k = pc.rx_hard_case(name, n, mod, True, nbytes, frames=2, seed=3)
    c = _ctx(api, name, n, mod, True)
    cap = np.concatenate([k["rx"][0], k["rx"][1], np.zeros(500, np.complex64)])
    x = c.to_device(cap)
    det = c.sc_scan_long(x, c.frame_samples(nbytes) - 3 * c.S, 16)
    assert det["d_hat"].size == 2 and not det["more"], det["d_hat"]
    got = c.decode_packets(x, det, k["D"])
    c.synchronize()
    disp = c.last_dispatch()
    assert "k_pkt_rows" in disp and "k_gather_rows" in disp and disp.endswith("k_pkt_finish"), disp
    with np.errstate(all="ignore"):
        want = P.packets(orc, cap, det, n, True, mod, k["D"], training=k["trn"])
    head = bytes(16)
    for i, w in enumerate(want):
        assert (int(got["status"][i]), int(got["offset"][i]), int(got["len"][i])) == (w["status"], w["offset"], w["len"]) and w["status"] == 0, (name, i)
        assert_bytes_match(head + bytes(got["bytes"][i, : w["len"]].cpu().numpy()), head + w["bytes"], w["soft"], mod, what=f"{name} packet {i}")
    assert got["f_delta"].cpu().numpy().tobytes() == det["f_delta"].tobytes() and got["metric"].cpu().numpy().tobytes() == det["metric"].tobytes()


@pytest.mark.parametrize("name", ["stdrng", "holes"])
def test_combine_under_the_table_is_its_composition(name):
    """decode_combine with R = 2 captures of every frame against tests/test_gpu_combine.py's composition of the stage entry points,
    both contexts built with the family's tables"""
    api = _api()
    n, mod, F, R, payload, ecc = 64, api.QAM64, 5, 2, 200, api.ECC_LDPC648
    kw = dict(_tables_kw(name, n), chest_mode=_chest_for(api, name))
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, **kw)
    c0 = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_NONE, **kw)
    g = torch.Generator(device=c.device)
    g.manual_seed(77)
    pay = torch.randint(0, 256, (F, payload), dtype=torch.uint8, device=c.device, generator=g)
    D = c.data_symbols(payload)
    rx = tcb._branch_captures(c, pay, R, [24.0, 20.0], 950)
    res = c.decode_combine(rx, max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch().split("+")
    assert "k_llr_combine" in trace and "k_linkq" in trace and "k_sym<llr>" in trace and ("k_chest_solve" in trace) == (name == "holes"), trace
    want, q, s = tcb._composition(api, c, c0, rx, D, rx.shape[2])
    assert torch.equal(res["quality"].view(F * R, -1), s["quality"]) and np.array_equal(res["weight"].view(-1).cpu().numpy(), q)
    assert_rows_are(res, want)
    good = [f for f, (st, n_out, data) in want.items() if st == 0 and bytes(data[:payload]) == bytes(pay[f].cpu().numpy())]
    print(f"{name}: statuses {[w[0] for w in want.values()]}, weights {q.tolist()}, {len(good)} of {F} whole")
    assert len(good) >= 3


# ---------------------------------------------------------------------------------------------------------- 8. isolation
def _isolation_calls(c, name):
    """{call: thunk -> tuple of tensors} on context c with the inputs of family `name`"""
    k = pc.rx_hard_case(name, 64, 4, True, 100, frames=4, seed=9)
    rx, D = c.to_device(k["rx"]), k["D"]
    off, fd = _i32(c, [w["offset"] for w in k["want"]]), _f64(c, [w["f_delta"] for w in k["want"]])
    pay = c.to_device(k["pay"])
    rng = np.random.default_rng(8)
    hk_in = c.to_device((1.0 + 0.3 * (rng.standard_normal((4, 64)) + 1j * rng.standard_normal((4, 64)))).astype(np.complex64))

    def decode():
        r = c.decode_batch(rx, max_symbols=D)
        rows = [r["bytes"][f, : int(r["len"][f])] for f in range(rx.shape[0])]
        return (r["status"], r["len"], r["offset"], r["f_delta"], r["metric"], *rows)

    return {
        "encode_batch": lambda: (c.encode_batch(pay),),
        "decode_batch": decode,
        "estimate_channel": lambda: (c.estimate_channel(rx, off, fd),),
        "chest_smooth": lambda: (c.chest_smooth(hk_in),),
        "rx_quality": lambda: (c.rx_quality(rx, D, n_points=c.frame_points(100), offset=off, f_delta=fd),),
        "cfo_wide": lambda: tuple(c.cfo_wide(rx, off, fd, 8).values()),
    }


def test_two_contexts_with_different_tables_do_not_share_them():
    """Two contexts with the same ofdm_params and different tables (stdrng, unit_loud), used alternately on one stream: every result is
    the result of a fresh context that did the same call alone.  Both creation orders: the per-context tables -- the header and its
    maximum, 1 / t, |t|^2 and R^-1, sum |t|^2, conj(t) -- must not live in anything keyed by the parameters."""
    api = _api()
    names = ("stdrng", "unit_loud")
    make = lambda name: _ctx(api, name, 64, api.QAM16, True)  # noqa: E731
    alone = {}
    for name in names:
        for call in _isolation_calls(make(name), name):
            fresh = make(name)
            alone[name, call] = _isolation_calls(fresh, name)[call]()
            fresh.synchronize()
    for a, b in (alone["stdrng", "encode_batch"], alone["unit_loud", "encode_batch"]), (alone["stdrng", "chest_smooth"], alone["unit_loud", "chest_smooth"]):
        assert not torch.equal(a[0], b[0])                            # (the tables do make a difference)
    for order in (names, names[::-1]):
        ctxs = {name: make(name) for name in order}
        calls = {name: _isolation_calls(ctxs[name], name) for name in order}
        for rnd in range(2):
            for call in calls[order[0]]:
                for name in (order if rnd == 0 else order[::-1]):
                    got = calls[name][call]()
                    ctxs[name].synchronize()
                    want = alone[name, call]
                    assert len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(got, want)), (order, rnd, name, call)


# ---------------------------------------------------------------------------------------------------------- 9. the free functions
def test_free_functions_take_explicit_tables(orc):
    """api.encode / decode / decode_long / decode_all with training= / preamble= arrays (the context cache used to raise TypeError:
    unhashable type on them): the payload comes back, equal to the Context path; the same arrays reuse one context, others get another"""
    api = _api()
    pre, trn = pc.tables("unit_loud", 64)
    rng = np.random.default_rng(31)
    pay = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    tx = api.encode(pay, True, api.QAM64, training=trn, preamble=pre)
    n_ctx = len(api._CTX_CACHE)
    c = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, preamble=pre, training=trn)
    want_tx = c.encode_batch(c.to_device(np.frombuffer(pay, np.uint8).reshape(1, -1).copy()))[0].cpu().numpy()
    assert np.array_equal(tx, want_tx.astype(np.complex128))
    assert rel_err(tx, orc.encode(pay, True, orc.QAM64, preamble=pre, training=trn)) <= TOL
    assert np.array_equal(api.encode(pay, True, api.QAM64, training=trn.copy(), preamble=pre.copy()), tx) and len(api._CTX_CACHE) == n_ctx
    other = api.encode(pay, True, api.QAM64, training=pc.tables("holes", 64)[1], preamble=pre)
    assert len(api._CTX_CACHE) == n_ctx + 1 and not np.array_equal(other, tx)
    cap = wide(through_channel(orc, rng, tx, tx.size + 400, 31, 0.004, snr_db=35.0, data_start=800))
    assert api.decode(cap, True, api.QAM64, training=trn) == pay
    r = c.decode_batch(c.to_device(cap).reshape(1, -1), max_symbols=c.data_symbols(len(pay)))
    assert int(r["status"][0]) == 0 and bytes(r["bytes"][0, : int(r["len"][0])].cpu().numpy()) == pay
    assert bytes(orc.decode_sc(cap, guard=True, modulation=orc.QAM64, training=trn)["bytes"]) == pay
    long = api.decode_long(cap, True, api.QAM64, training=trn, preamble=pre)
    assert long["status"] == 0 and bytes(long["bytes"][: long["len"]].cpu().numpy()) == pay
    every = api.decode_all(cap, True, api.QAM64, training=trn, preamble=pre, holdoff=tx.size - 240, max_symbols=c.data_symbols(len(pay)))
    assert len(every) == 1 and every[0]["status"] == 0 and every[0]["bytes"] == pay
