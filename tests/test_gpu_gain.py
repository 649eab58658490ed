"""Every receive kernel gives ONE answer at any input gain.  The same capture is handed to the library at the gains of
tests/gain_cases.py (2^-20 .. 2^20 around a unit-peak frame, and -1), scaled by one exact f32 multiplication; the run at g = 1 is the
baseline of every row, and must itself be right first (status 0 and the payload back, or the f64 oracle's lag / bytes), so that two
equal wrong answers cannot pass.  Every other gain must then return the baseline's BITS: decisions (lags, statuses, m, bytes, the
slow-list and redo-list counts) equal, CFOs, metrics, soft points and LLRs bit-identical, and the quantities that are amplitudes or
powers by definition exactly g (H, the xcorr peak: |out|) or g^2 (noise_var, gain, the wide-CFO window energies) times the baseline's.
tests/test_gain_cpu.py shows that the f64 definitions have this property; there is no tolerance and no excused share in this file.
Every row that has a dispatch trace names the kernel it means to test through last_dispatch().

Where a kernel takes a channel estimate, the one given at gain g is g times the baseline's (made by the same exact multiplication, not
by the library, so that a red channel-estimate row does not colour the demodulator rows).  k_demod64's burst instantiations take no
channel estimate at all, so their output is by definition not invariant: the burst row runs them at g = 1 and holds k_demod64<HK> on
g x with the flat channel hk = g to their bytes.

Shapes: tools/link.py's seeded link (FIR channel, delay, CFO, noise), 5 frames a batch (3 from N = 1024 on), payload 100 bytes at
N = 64 and 300 above, the last slot noise only, rows an odd number of samples apart wherever the kernel under test is reached by such
rows: the k_sc_tile, k_sc_stream and k_scb_* rows run on even and on odd rows, k_sc80 has a row of tight odd rows of its own (their
last one leaves it), and only the one-tile filters k_sc_cf, which take even rows alone, never see odd ones.  The stand-alone xcorr and
frequency_correction entry points write no dispatch trace; the SYNC_REFERENCE chain that runs both names them.

Out of scope: the transmit side normalises its own output, so no input gain reaches it; and channel_batch is not homogeneous bit for
bit (the complex square root of its pseudo-variance is not), so the captures are scaled behind it."""
import functools
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc16_ref  # noqa: E402
import soft_ref as sr  # noqa: E402
from chain_refs import ALL_MODES, mode_layers  # noqa: E402
from gain_cases import GAINS, same, scaled, times  # noqa: E402
from tools.link import branch_link_on, data_snr, link as _link, wide_link_on  # noqa: E402
from util import assert_bytes_match, make_symbols_np, wide  # noqa: E402

pytestmark = pytest.mark.gpu

WLS, CFO_WIDE, SYNC_REFERENCE = 1, 3, 1


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def frames_of(n):
    return 5 if n < 1024 else 3


def payload_of(n):
    return 100 if n == 64 else 300


def link_snr(n):
    """uncoded 64-QAM must come back whole for the baseline to be right: 40 dB on the data symbols at every N"""
    return data_snr(n, 40.0)


def noise_rows(c, rows, span, seed, sigma=0.01):
    import torch

    g = torch.Generator(device=c.device)
    g.manual_seed(seed)
    return sigma * torch.view_as_complex(torch.randn((rows, span, 2), dtype=torch.float32, device=c.device, generator=g))


def odd_rows_noise_last(c, rx, seed):
    """the link's captures with one more (zero) sample a row, so that rows lie an odd number of samples apart, and the last slot noise only"""
    import torch

    rx = torch.cat([rx, torch.zeros_like(rx[..., :1])], dim=-1)
    rx[-1] = noise_rows(c, 1, rx.shape[-1], seed).reshape(rx[-1].shape) if rx.dim() == 2 else noise_rows(c, rx.shape[1], rx.shape[-1], seed)
    assert rx.shape[-1] % 2 == 1
    return rx.contiguous()


def link_case(api, ecc, n, mod, seed, wide_cfo=False, **ctx_kw):
    """(context, payloads, captures [frames, odd span] with the last slot noise only, data symbols[, the m drawn per frame])"""
    F, p = frames_of(n), payload_of(n)
    if wide_cfo:
        c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, **ctx_kw)
        pay, rx, m, _ = wide_link_on(c, F, p, link_snr(n), seed)
        return c, pay, odd_rows_noise_last(c, rx, seed), c.data_symbols(p), host(m)
    c, pay, rx, D = _link(ecc, n, mod, F, p, link_snr(n), seed, guard=True, **ctx_kw)
    return c, pay, odd_rows_noise_last(c, rx, seed), D


def assert_delivered(r, pay, what):
    """the baseline is right: every frame but the noise-only slot has status 0 and the payload in front; the slot has no frame"""
    st, by, p = host(r["status"]), host(r["bytes"]), host(pay)
    assert st.ndim == 1 and np.all(st[:-1] == 0) and st[-1] != 0, (what, st)
    assert np.all(host(r["len"])[:-1] >= p.shape[1]) and np.array_equal(by[:-1, :p.shape[1]], p[:-1]), what


def assert_same_decode(got, base, what, extra_int=(), metric_times=1.0):
    """metric_times: the power of |g| the chain's metric scales with by definition (Schmidl-Cox: a ratio, 1)"""
    for k in ("status", "len", "offset") + tuple(extra_int):
        assert np.array_equal(host(got[k]), host(base[k])), (what, k, host(got[k]), host(base[k]))
    assert same(got["f_delta"], base["f_delta"]), (what, "f_delta", host(got["f_delta"]), host(base["f_delta"]))
    assert same(got["metric"], times(base["metric"], metric_times)), (what, "metric", host(got["metric"]), host(base["metric"]))
    ln, gb, bb = np.atleast_1d(host(base["len"])), host(got["bytes"]), host(base["bytes"])
    gb, bb = gb.reshape(ln.size, -1), bb.reshape(ln.size, -1)
    for f in range(ln.size):
        assert bytes(gb[f, :ln[f]]) == bytes(bb[f, :ln[f]]), (what, f)


# ------------------------------------------------------------------------------------------------ 1. the Schmidl-Cox families
class Verdicts(dict):
    """{n_lags: [orc.sc_sync per capture]}, computed when first asked for"""

    def __init__(self, orc, caps, S):
        super().__init__()
        self.orc, self.caps, self.S = orc, caps, S

    def __missing__(self, lags):
        self[lags] = [self.orc.sc_sync(wide(row), self.S, 3, lags, 0.5) for row in self.caps]
        return self[lags]


@functools.lru_cache(maxsize=None)
def sc_captures(orc, n, mod, odd=False):
    """[frames, span] complex64 on the host: the link's captures laid on a noise floor -- ordinary ones, the second a late packet (its
    delay beyond the peak window W = 3 S), the last slot noise only -- and the oracle's verdicts {n_lags: [orc.sc_sync]} (0: the whole
    slot).  odd: the same captures without their last sample, so that the rows lie an odd number of samples apart."""
    S = n + n // 4
    c, _, rx, _ = _link(0, n, mod, frames_of(n), payload_of(n), link_snr(n), 700 + n, guard=True)
    rx = host(rx)
    late = 3 * S + 40 if n > 64 else 640      # (N = 64: also beyond the first launch of the two-launch search, 576 lags)
    span = max(rx.shape[1] + late + 64, 2176)
    rng = np.random.default_rng(n)
    caps = 0.003 * (rng.standard_normal((rx.shape[0], span)) + 1j * rng.standard_normal((rx.shape[0], span)))
    for f in range(rx.shape[0] - 1):
        at = late if f == 1 else 0
        caps[f, at:at + rx.shape[1]] += rx[f]
    caps = np.ascontiguousarray(caps.astype(np.complex64)[:, :span - 1 if odd else span])
    assert caps.shape[1] % 2 == int(odd)
    want = Verdicts(orc, caps, S)
    d = [w[0] for w in want[0]]
    assert all(S < x <= 2 * S for i, x in enumerate(d[:-1]) if i != 1) and d[1] > late and d[-1] == -1, d       # each kind is what it is meant to be
    assert want[2 * S][1][0] != d[1]                                                                            # the bounded search ends before the late packet
    return caps, want


starts = lambda *prefixes: (lambda disp: disp.startswith(prefixes))
SC_FAMILIES = [
    # id, N, modulation, tuning, {n_lags in units of S (0: the whole slot, else a bounded search): predicate on last_dispatch()}, odd rows too
    ("sc80", 64, 6, {}, {0: starts("k_sc80"), 2: starts("k_sc80")}, False),                       # (odd rows: test_sc80_rows_of_odd_length)
    ("sc_cf_one_launch", 64, 6, {"no_sc80": 1, "sc_first_lags": 0}, {0: starts("k_sc_cf<256>+"), 2: starts("k_sc_cf<128>+")}, False),
    # two launches need 2 x 576 lags or more and the 256-chunk tile (more than 960 lags): the bounded search is one over 15 S = 1 200 lags,
    # with the late packet's crossing behind the first launch's 576
    ("sc_cf_two_launches", 64, 6, {"no_sc80": 1}, {0: starts("k_sc_cf<128,first>+k_sc_cf<256,list>"),
                                                   15: starts("k_sc_cf<128,first>+k_sc_cf<256,list>")}, False),
    ("sc_tile", 1024, 2, {"no_sc_stream": 1, "no_sc_big": 1}, {0: starts("k_sc_tile<cross>+k_sc_tile<peak>"), 2: lambda d: d == "k_sc_tile"}, True),
    ("sc_stream256", 256, 4, {}, {0: starts("k_sc_stream"), 2: starts("k_sc_stream")}, True),
    ("sc_stream1024", 1024, 2, {}, {0: starts("k_sc_stream"), 2: starts("k_sc_stream")}, True),
    ("scb2048", 2048, 4, {"no_sc_stream": 1}, {0: lambda d: d.startswith("k_scb_chunks") and "+k_scb_fine" in d,
                                               2: lambda d: d.startswith("k_scb_chunks") and "+k_scb_fine" in d}, True),
]
SC_ROWS = [(f[0] + ("_odd_rows" if odd else ""),) + f[1:5] + (odd,) for f in SC_FAMILIES for odd in ((False, True) if f[5] else (False,))]


@pytest.mark.parametrize("n,mod,tuning,forms,odd", [r[1:] for r in SC_ROWS], ids=[r[0] for r in SC_ROWS])
def test_schmidl_cox_families(api, orc, n, mod, tuning, forms, odd):
    caps, want = sc_captures(orc, n, mod, odd)
    assert caps.shape[1] % 2 == int(odd)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True, tuning=tuning)
    x1 = ctx.to_device(caps)
    wrong = []
    for form, names_family in forms.items():
        lags = form * S

        def run(x):
            out = ctx.sc_correlate(x, n_lags=lags)
            assert names_family(ctx.last_dispatch()), (n, tuning, lags, ctx.last_dispatch())
            return out, ctx.last_dispatch(), ctx.get_tuning("stat_sc_slow_frames"), ctx.get_tuning("stat_sc_redo_frames")

        base, disp, slow, redo = run(x1)
        print(f"N = {n} {tuning} {'odd' if odd else 'even'} rows, n_lags = {lags}: {disp}; slow-list frames {slow}, redo-list frames {redo} at g = 1")
        assert [int(d) for d in host(base[0])] == [w[0] for w in want[lags]], (n, tuning, lags, host(base[0]))
        assert "k_sc_cf<256,list>" not in disp or redo == 2, redo      # the late packet and the noise-only slot, and no other
        for g in GAINS:
            got, gdisp, gslow, gredo = run(scaled(x1, g))
            ok = gdisp == disp and np.array_equal(host(got[0]), host(base[0])) and same(got[1], base[1]) and same(got[2], base[2]) and \
                (gslow, gredo) == (slow, redo)
            if not ok:
                wrong.append((lags, g, gdisp, host(got[0]).tolist(), gslow, gredo))
                print(f"  wrong at g = {g}: {gdisp}; d_hat {host(got[0]).tolist()} (g = 1: {host(base[0]).tolist()}), slow {gslow}, redo {gredo}; "
                      f"f_delta same {same(got[1], base[1])}, metric same {same(got[2], base[2])}")
    assert not wrong, wrong


def test_sc80_rows_of_odd_length(api, orc):
    """tight rows of odd length: k_sc80 takes all but the last row, which goes through the general path on its own"""
    caps, _ = sc_captures(orc, 64, 6)
    caps = caps[:, :-1]
    ctx = api.Context(n_fft=64, modulation=6, guard_bands=True)
    x1 = ctx.to_device(np.ascontiguousarray(caps))
    base = ctx.sc_correlate(x1)
    disp = ctx.last_dispatch()
    assert disp.startswith("k_sc80") and [int(d) for d in host(base[0])] == [orc.sc_sync(wide(r), 80, 3, 0, 0.5)[0] for r in caps]
    for g in GAINS:
        got = ctx.sc_correlate(scaled(x1, g))
        assert ctx.last_dispatch() == disp and np.array_equal(host(got[0]), host(base[0])) and same(got[1], base[1]) and same(got[2], base[2]), g


def f64_bits(v):
    return struct.pack("<d", v)


def test_long_capture_search_reference_timing_and_frequency_correction(api, orc):
    """ofdm_sc_correlate_long over several slices from lag_lo > 0; ofdm_xcorr_batch (idx_max equal, peak = |out[idx_max]|: exactly |g|
    times the baseline's, the locking signal being the library's own and not scaled); ofdm_frequency_correction_batch (an angle: the same
    bits).  Neither stage entry point writes a dispatch trace; the decode chain under SYNC_REFERENCE, which runs both, names them."""
    caps, want = sc_captures(orc, 64, 6)
    ctx = api.Context(n_fft=64, modulation=6, guard_bands=True)
    rng = np.random.default_rng(5)
    long_cap = np.concatenate([(0.003 * (rng.standard_normal(4001) + 1j * rng.standard_normal(4001))).astype(np.complex64), caps[0]])
    x1 = ctx.to_device(long_cap)
    lag_lo = 1001
    base = ctx.sc_correlate_long(x1, lag_lo=lag_lo, slice_lags=1024)
    disp = ctx.last_dispatch()
    wd, _, wm, wfd = orc.sc_sync(wide(long_cap[lag_lo:]), 80, 3, 0, 0.5)
    # four slices of 1 024 lags in one batch, the tail slice, and the slice with the crossing again with its whole peak window: k_sc80 each
    assert disp == "+".join(["k_sc80+k_sc_tile<list>"] * 3), disp
    assert base[0] == lag_lo + wd == 4001 + want[0][0][0] and abs(base[1] - wfd) <= 1e-9
    for g in GAINS:
        got = ctx.sc_correlate_long(scaled(x1, g), lag_lo=lag_lo, slice_lags=1024)
        assert ctx.last_dispatch() == disp and got[0] == base[0] and f64_bits(got[1]) == f64_bits(base[1]) and \
            np.float32(got[2]).tobytes() == np.float32(base[2]).tobytes(), (g, got, base)
    # the reference's own detector pair
    lock = ctx.to_device(orc.locking_signal(80))
    xc = ctx.to_device(caps)
    idx, pk = ctx.xcorr(xc, lock)
    wi = [orc.xcorr_fft(wide(r), orc.locking_signal(80))[0] for r in caps[:-1]]
    assert host(idx)[:-1].tolist() == wi
    S = 80
    off = host(idx).astype(np.int64) - caps.shape[1]
    at = np.clip(off, 0, caps.shape[1] - 5 * S)
    lr = np.stack([caps[f, at[f] + 3 * S: at[f] + 5 * S] for f in range(caps.shape[0])])
    fd = ctx.frequency_correction(ctx.to_device(lr))
    for f in range(caps.shape[0] - 1):
        assert abs(host(fd)[f] - orc.frequency_correction(wide(lr[f, :S]), wide(lr[f, S:]))) <= 1e-12
    for g in GAINS:
        gi, gp = ctx.xcorr(scaled(xc, g), lock)
        assert np.array_equal(host(gi), host(idx)) and same(gp, times(pk, abs(g))), g
        assert same(ctx.frequency_correction(scaled(ctx.to_device(lr), g)), fd), g
    ref = api.Context(n_fft=64, modulation=6, guard_bands=True, sync_mode=SYNC_REFERENCE, cfo_mode=api.CFO_ABS)
    _, pay, rx, D = link_case(api, 0, 64, 6, 770)
    base = ref.decode_batch(rx, max_symbols=D)
    disp = ref.last_dispatch()
    assert disp.startswith("k_xcorr+k_rx_prepare_ref+k_freq_corr"), disp
    for f, row in enumerate(host(rx)):          # the baseline is the oracle's decode_ref: the reference's detectors lose the CFO's sign
        w = orc.decode_ref(wide(row), True, 6, 64)
        assert (int(base["status"][f]), int(base["offset"][f])) == (w["status"], w["offset"]), (f, w["status"], w["offset"])
        assert w["status"] != 0 or abs(float(base["f_delta"][f]) - w["f_delta"]) <= 1e-9, f
    assert int((host(base["status"]) == 0).sum()) >= 3
    for g in GAINS:
        got = ref.decode_batch(scaled(rx, g), max_symbols=D)
        assert ref.last_dispatch() == disp
        assert_same_decode(got, base, ("reference sync", g), metric_times=abs(g))    # this chain's metric is the xcorr peak |out[idx_max]|


# ------------------------------------------------------------------------------------------------ 2. channel estimates
@pytest.mark.parametrize("n,mod", [(64, 6), (256, 4), (1024, 2)])
def test_channel_estimates_scale_with_the_capture(api, n, mod):
    """H(g x) == g H(x) bit for bit under CHEST_LS and CHEST_WLS, and chest_smooth(g H) == g chest_smooth(H)"""
    c, pay, rx, D = link_case(api, 0, n, mod, 800 + n)
    r = c.decode_batch(rx, max_symbols=D)
    assert_delivered(r, pay, n)
    off, fd = r["offset"], r["f_delta"]
    for mode, name in ((0, "k_sym<chest>"), (WLS, "k_chest_solve")):
        ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True, chest_mode=mode)
        h1 = ctx.estimate_channel(rx, off, fd)
        disp = ctx.last_dispatch()
        assert "k_sym<chest>" in disp and name in disp and ("k_chest_solve" in disp) == (mode == WLS), disp
        assert np.isfinite(host(h1)).all() and np.abs(host(h1)[:-1]).min() > 0
        s1 = ctx.chest_smooth(h1)
        sdisp = ctx.last_dispatch()
        assert "k_chest_solve" in sdisp, sdisp
        for g in GAINS:
            hg = ctx.estimate_channel(scaled(rx, g), off, fd)
            assert ctx.last_dispatch() == disp and same(hg, times(h1, g)), (n, mode, g)
            assert same(ctx.chest_smooth(scaled(h1, g)), times(s1, g)) and ctx.last_dispatch() == sdisp, (n, mode, g, "smooth")


# ------------------------------------------------------------------------------------------------ 3. rx_demod and rx_llr
@functools.lru_cache(maxsize=None)
def symbol_streams(orc, n, mod, frames, syms):
    """(x [frames, syms S + 1] fc32 through a per-frame channel, the same symbols through frame 0's channel for all, h [frames, n] fc32,
    the oracle's (bytes, soft) per frame for both)"""
    rng = np.random.default_rng([n, mod, frames, syms])
    S = n + n // 4
    x, _ = make_symbols_np(orc, rng, frames * syms, n, True, mod, snr_db=34.0)
    h = (1.0 + 0.2 * (rng.standard_normal((frames, n)) + 1j * rng.standard_normal((frames, n)))).astype(np.complex64)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros((frames, 1), np.complex64)], axis=1))     # an odd row stride
    per_frame = sr.through_h(x.reshape(frames, syms * S), n, wide(h))
    shared = sr.through_h(x.reshape(frames, syms * S), n, wide(h[:1]))
    ref = lambda rows, hf: [orc.rx_demod(wide(rows[f]), n, True, mod, hk=wide(hf(f)), want_soft=True) for f in range(frames)]
    return pad(per_frame), pad(shared), h, ref(per_frame, lambda f: h[f]), ref(shared, lambda f: h[0])


DEMOD_ROWS = [
    # id, entry point, N, frames, symbols, dispatch, per-frame H too
    ("k_demod64", "bytes", 64, 5, 8, "k_demod64", False),            # 5 groups: the plain instantiation; k_demod64 takes a shared H only
    ("k_demod_mid256", "bytes", 256, 5, 3, "k_demod_mid", True),
    ("k_demod_mid2048", "bytes", 2048, 3, 2, "k_demod_mid", True),
    ("k_demod4096", "bytes", 4096, 3, 2, "k_demod4096", True),
    ("k_sym_demod64", "soft", 64, 5, 3, "k_sym<demod>", True),
    ("k_sym_demod1024", "soft", 1024, 3, 2, "k_sym<demod>", True),
    ("k_sym_llr64", "llr", 64, 5, 3, "k_sym<llr>", True),
    ("k_sym_llr1024", "llr", 1024, 3, 2, "k_sym<llr>", True),
]


@pytest.mark.parametrize("entry,n,frames,syms,kernel,per_frame", [r[1:] for r in DEMOD_ROWS], ids=[r[0] for r in DEMOD_ROWS])
def test_demod_and_llr(api, orc, entry, n, frames, syms, kernel, per_frame):
    """x -> g x with hk -> g hk: bytes, soft points and int8 LLRs bit-identical; modulations 2, 6, 8"""
    for mod in (2, 6, 8):
        xp, xs, h, ref_p, ref_s = symbol_streams(orc, n, mod, frames, syms)
        ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True)
        for what, x, hk, ref in (("per frame", xp, h, ref_p), ("shared", xs, h[0], ref_s)):
            if what == "per frame" and not per_frame:
                continue
            x1, h1 = ctx.to_device(x), ctx.to_device(np.ascontiguousarray(hk))

            def run(xd, hd):
                if entry == "llr":
                    out = (ctx.rx_llr(xd, syms, hk=hd),)
                elif entry == "soft":
                    out = ctx.rx_demod(xd, syms, hk=hd, want_soft=True)
                else:
                    out = (ctx.rx_demod(xd, syms, hk=hd),)
                assert ctx.last_dispatch() == kernel, (ctx.last_dispatch(), kernel, mod, what)
                return out

            base = run(x1, h1)
            want_bytes = b"".join(r[0] for r in ref)
            wsoft = np.concatenate([r[1] for r in ref])
            if entry == "llr":      # the baseline is right: every LLR that is not small carries the sign of the oracle's hard bit
                L = host(base[0]).reshape(-1)
                hard = sr.unpack_bits(np.frombuffer(want_bytes, np.uint8))
                assert np.array_equal((L > 0)[np.abs(L) >= 4], (hard == 1)[np.abs(L) >= 4]) and np.abs(L).max() >= 16
            else:
                assert_bytes_match(bytes(host(base[0]).reshape(-1)), want_bytes, wsoft, mod, what=f"{kernel} N {n} mod {mod} {what}")
            for g in GAINS:
                got = run(scaled(x1, g), scaled(h1, g))
                assert all(same(a, b) for a, b in zip(got, base)), (kernel, n, mod, what, g)


def test_demod64_bursts_are_the_flat_channel(api, orc):
    """k_demod64<burst*> has no channel input: x at g = 1 is its whole domain here.  k_demod64<HK> on g x with the flat channel
    hk = g (equalising by a real power of two is exact) must give the burst kernel's bytes, and the oracle's."""
    rng = np.random.default_rng(640)
    x, _ = make_symbols_np(orc, rng, 4 * 8, 64, True, 6, snr_db=34.0)
    want, wsoft = orc.rx_demod(wide(x), 64, True, 6, want_soft=True)
    ctx = api.Context(n_fft=64, modulation=6, guard_bands=True)
    x1 = ctx.to_device(x.reshape(4, 640))
    base = ctx.rx_demod(x1, 8)
    assert ctx.last_dispatch() == "k_demod64<burst4>", ctx.last_dispatch()
    assert_bytes_match(bytes(host(base).reshape(-1)), want, wsoft, 6, what="burst4")
    ones = ctx.to_device(np.ones(64, np.complex64))
    for g in (1.0,) + GAINS:
        got = ctx.rx_demod(scaled(x1, g), 8, hk=scaled(ones, g))
        assert ctx.last_dispatch() == "k_demod64" and same(got, base), g


# ------------------------------------------------------------------------------------------------ 4. link quality, wide CFO
Q_SAME, Q_SQUARE = (0, 3, 4, 5, 6), (1, 2)      # valid, snr, llr_unit, evm2, points | noise_var, gain


def assert_same_quality(got, base, g, what):
    got, base = host(got).reshape(-1, 8), host(base).reshape(-1, 8)
    for k in Q_SAME:
        assert same(got[:, k], base[:, k]), (what, g, "field", k, got[:, k], base[:, k])
    for k in Q_SQUARE:
        assert same(got[:, k], times(base[:, k], g * g)), (what, g, "field", k, got[:, k], base[:, k])


@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 2)])
def test_link_quality(api, n, mod):
    c, pay, rx, D = link_case(api, 0, n, mod, 900 + n)
    r = c.decode_batch(rx, max_symbols=D)
    assert_delivered(r, pay, n)
    off, fd = r["offset"], r["f_delta"]
    h1 = c.estimate_channel(rx, off, fd)
    n_points = c.frame_points(payload_of(n))
    base = c.rx_quality(rx, D, 10, n_points, off, fd, h1)
    assert c.last_dispatch() == "k_linkq"
    q = host(base)
    assert np.all(q[:-1, 0] == 1) and np.all(q[:-1, 6] == n_points) and np.all(q[:-1, 3] > 100) and np.all((0 < q[:-1, 5]) & (q[:-1, 5] < 0.05)), q
    for g in GAINS:
        got = c.rx_quality(scaled(rx, g), D, 10, n_points, off, fd, scaled(h1, g))
        assert c.last_dispatch() == "k_linkq"
        assert_same_quality(got, base, g, n)


@pytest.mark.parametrize("n,mod", [(64, 6), (128, 4), (1024, 2)], ids=["64", "128_shuffle", "1024_workgroup"])
def test_wide_cfo(api, n, mod):
    c, pay, rx, D, m = link_case(api, 0, n, mod, 1000 + n, wide_cfo=True)
    r = c.decode_batch(rx, max_symbols=D)            # (cfo_mode SIGNED: the Schmidl-Cox offset and its wrapped CFO)
    off, fd = r["offset"], r["f_delta"]
    base = c.cfo_wide(rx, off, fd)
    assert c.last_dispatch() == "k_cfo_wide"
    assert np.array_equal(host(base["m"])[:-1], m[:-1]) and np.any(m[:-1] != 0), (host(base["m"]), m)
    for g in GAINS:
        got = c.cfo_wide(scaled(rx, g), off, fd)
        assert c.last_dispatch() == "k_cfo_wide"
        assert np.array_equal(host(got["m"]), host(base["m"])) and same(got["f_delta"], base["f_delta"]), (n, g)
        assert same(got["metric"], times(base["metric"], g * g)), (n, g, host(got["metric"]), host(base["metric"]))


# ------------------------------------------------------------------------------------------------ 5. the decode chains
def chain_kernel(n, ecc, ctx_kw):
    """a kernel the chain of this row must have run"""
    inner = mode_layers(ecc)[2]
    if inner not in (0, 1):
        return "k_sym<llr>"
    if ctx_kw.get("chest_mode") == WLS:
        return "k_chest_solve"
    return {64: "k_rxframe64", 1024: "k_rxframe1024", 4096: "k_demod4096<frame>"}.get(n, "k_demod_mid<frame>")


def decode_row(api, ecc, n, mod, seed, **ctx_kw):
    wide_cfo = ctx_kw.get("cfo_mode") == CFO_WIDE
    case = link_case(api, ecc, n, mod, seed, wide_cfo=wide_cfo, **ctx_kw)
    c, pay, rx, D = case[:4]
    base = c.decode_batch(rx, max_symbols=D)
    disp = c.last_dispatch()
    assert chain_kernel(n, ecc, ctx_kw) in disp and (not wide_cfo or "k_cfo_wide" in disp), (ecc, n, disp)
    assert_delivered(base, pay, (ecc, n, ctx_kw))
    if wide_cfo:
        assert np.any(case[4][:-1] != 0)
    for g in GAINS:
        got = c.decode_batch(scaled(rx, g), max_symbols=D)
        assert c.last_dispatch() == disp, (ecc, n, g, c.last_dispatch(), disp)
        assert_same_decode(got, base, (ecc, n, ctx_kw, g))


@pytest.mark.parametrize("ecc", ALL_MODES)
def test_decode_batch_every_mode(api, ecc):
    decode_row(api, ecc, 64, 6, 1100 + ecc)


@pytest.mark.parametrize("ecc", [0, 2, 12, 16, 96])
@pytest.mark.parametrize("n,mod", [(256, 4), (1024, 2), (4096, 4)])
def test_decode_batch_other_lengths(api, n, mod, ecc):
    decode_row(api, ecc, n, mod, 1200 + n + ecc)


@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 2)])
@pytest.mark.parametrize("ctx_kw", [{"chest_mode": WLS}, {"cfo_mode": CFO_WIDE}], ids=["chest_wls", "cfo_wide"])
def test_decode_batch_receive_modes(api, n, mod, ctx_kw):
    decode_row(api, 0, n, mod, 1300 + n, **ctx_kw)


def test_host_and_long_capture_entry_points(api):
    """ofdm_rx_decode_host in chunks of 2, ofdm_rx_decode_long and ofdm_rx_decode_long_host, N = 64"""
    c, pay, rx, D = link_case(api, 0, 64, 6, 1400)
    x = host(rx)
    base = c.decode_host(x, max_symbols=D, chunk_frames=2)
    disp = c.last_dispatch()
    assert "k_rxframe64" in disp, disp
    assert_delivered(base, pay, "decode_host")
    for g in GAINS:
        got = c.decode_host(scaled(x, g), max_symbols=D, chunk_frames=2)
        assert c.last_dispatch() == disp
        assert_same_decode(got, base, ("decode_host", g))
    as_rows = lambda r: {k: (host(v).reshape(1, -1) if k == "bytes" else np.array([v])) for k, v in r.items()}
    cap = rx[0].contiguous()
    for name, call in (("decode_long", lambda v: c.decode_long(v, D)), ("decode_long_host", lambda v: c.decode_long_host(host(v), D))):
        base = as_rows(call(cap))
        disp = c.last_dispatch()
        assert "k_rx_prepare" in disp and "k_rxframe64" in disp and base["status"][0] == 0 and bytes(base["bytes"][0, :100]) == bytes(host(pay)[0]), (name, disp)
        for g in GAINS:
            got = as_rows(call(scaled(cap, g)))
            assert c.last_dispatch() == disp
            assert_same_decode(got, base, (name, g))


def test_decode_combine(api):
    """R = 2 captures of every frame, LDPC(648), N = 64: also branch_status and weight identical, quality as in the rx_quality row"""
    c = api.Context(n_fft=64, modulation=2, guard_bands=True, ecc=16)
    pay, rx = branch_link_on(c, 5, 100, (18.0, 14.0), 1500)
    rx = odd_rows_noise_last(c, rx, 1500)
    D = c.data_symbols(100)
    base = c.decode_combine(rx, max_symbols=D)
    disp = c.last_dispatch()
    assert "k_llr_combine" in disp and "k_linkq" in disp and "k_sym<llr>" in disp and "k_ldpc_decode" in disp, disp
    assert_delivered(base, pay, "combine")
    assert np.all(host(base["branch_status"])[:-1] == 0) and np.all(host(base["weight"])[:-1] > 0) and len(set(host(base["weight"])[:-1].ravel())) > 1
    for g in GAINS:
        got = c.decode_combine(scaled(rx, g), max_symbols=D)
        assert c.last_dispatch() == disp
        assert_same_decode(got, base, ("combine", g), extra_int=("branch_status", "weight"))
        assert_same_quality(got["quality"], base["quality"], g, "combine")


# ------------------------------------------------------------------------------------------------ 6. sc16: `scale` is such a gain
SC16_K = (-15, 0, 15, 20)          # scale = 2^-15 2^k; k = 15 is scale = 1.0, raw counts


def test_sc16_demod_scales(api, orc):
    """k_demod64_sc16 (shared H) and the widen fallback (per-frame H with soft points) on one fixed int16 stream, hk = 2^k hk_1"""
    xp, xs, h, _, _ = symbol_streams(orc, 64, 6, 5, 8)
    ctx = api.Context(n_fft=64, modulation=6, guard_bands=True)
    at_unit_scale = 2.0 ** -15
    for what, x, hk, kw, kernel in (("fused", xs, h[0], {}, "k_demod64_sc16"), ("widen", xp, h, {"want_soft": True}, "k_sc16_widen+k_sym<demod>")):
        q, s = sc16_ref.quantise(x, 0.9)
        hk1 = (np.ascontiguousarray(hk) * np.complex64(1.0 / (32768.0 * float(s)))).astype(np.complex64)
        qd, hd = ctx.to_device(q), ctx.to_device(hk1)
        base = None
        for k in SC16_K:
            scale = 2.0 ** (k - 15)
            hk_k = scaled(hd, 2.0 ** k)
            got = ctx.rx_demod_sc16(qd, 8, hk=hk_k, scale=scale, **kw)
            assert ctx.last_dispatch() == kernel, (what, ctx.last_dispatch())
            got = got if isinstance(got, tuple) else (got,)
            want = ctx.rx_demod(ctx.to_device(sc16_ref.widen(q, np.float32(scale))), 8, hk=hk_k, **kw)
            want = want if isinstance(want, tuple) else (want,)
            assert all(same(a, b) for a, b in zip(got, want)), (what, k, "the fc32 call on the widened samples")
            base = got if base is None else base
            assert all(same(a, b) for a, b in zip(got, base)), (what, k)
        # the baseline is right: the f64 oracle on the widened samples of every row (without the pad sample) with hk_1
        xw = wide(sc16_ref.widen(q, np.float32(at_unit_scale)))[:, :8 * 80]
        ref = [orc.rx_demod(xw[f], 64, True, 6, hk=wide(hk1 if hk1.ndim == 1 else hk1[f]), want_soft=True) for f in range(5)]
        assert_bytes_match(bytes(host(base[0]).reshape(-1)), b"".join(r[0] for r in ref), np.concatenate([r[1] for r in ref]), 6, what=f"sc16 {what}")


@pytest.mark.parametrize("ecc", [0, 80], ids=["none", "ldpc648fcs"])
def test_sc16_decode_scales(api, ecc):
    """decode_batch_sc16 and decode_long_sc16 on one fixed int16 capture, quantised at 0.9 of full scale"""
    c, pay, rx, D = link_case(api, ecc, 64, 6, 1600 + ecc)
    q, _ = sc16_ref.quantise(host(rx), 0.9)
    qd = c.to_device(q)
    base = base_long = None
    for k in (0,) + SC16_K:
        scale = 2.0 ** (k - 15)
        got = c.decode_batch_sc16(qd, max_symbols=D, scale=scale)
        disp = c.last_dispatch()
        assert disp.startswith("k_sc16_widen+"), disp
        want = c.decode_batch(c.to_device(sc16_ref.widen(q, np.float32(scale))), max_symbols=D)
        assert_same_decode(got, want, ("sc16 against the fc32 call", ecc, k))
        if base is None:
            base = got
            assert_delivered(base, pay, ("sc16", ecc))
        assert_same_decode(got, base, ("sc16", ecc, k))
        lg = c.decode_long_sc16(qd[0].contiguous(), D, scale=scale)
        assert "k_sc16_widen" in c.last_dispatch()
        as_rows = lambda r: {k_: (host(v).reshape(1, -1) if k_ == "bytes" else np.array([v])) for k_, v in r.items()}
        lg = as_rows(lg)
        assert_same_decode(lg, as_rows(c.decode_long(c.to_device(sc16_ref.widen(q[0], np.float32(scale))), D)), ("sc16 long against the fc32 call", ecc, k))
        if base_long is None:
            base_long = lg
            assert lg["status"][0] == 0 and bytes(lg["bytes"][0, :100]) == bytes(host(pay)[0])
        assert_same_decode(lg, base_long, ("sc16 long", ecc, k))
