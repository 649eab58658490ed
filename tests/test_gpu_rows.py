"""The row contract of the core entry points (include/ofdm_hip.h): rows are (base, stride, length), and the answer does not depend on
base or stride.  ofdm_amd/api.py only ever passes contiguous tensors with stride == row width; here every call goes to ctx.lib through
the ctypes callers of tests/rows.py with explicit strides, into flat buffers that hold a fixed fill everywhere outside the rows.

The rule of every case (that of tests/test_gpu_gain.py):
  - the dense call comes first and is itself right against the f64 oracle by the existing bars: bytes exactly (decision_margin >= 1e-4
    is asserted on the oracle's soft points, so assert_bytes_match may excuse nothing), lags and statuses exactly, CFO 1e-9 (1e-12 for
    frequency_correction), metric 1e-6 max(1, metric), samples norm-relative TOL = 1e-5;
  - every other layout gives the dense call's byte outputs exactly, and its float outputs bit for bit where last_dispatch() names the
    same kernels; where the layout sends the call to another kernel the floats are within the same TOL of the oracle;
  - everything outside the rows is untouched, inputs included; no tolerance is new;
  - every layout asserts its last_dispatch() string, read off the launchers' envelope conditions (the *_expect functions below restate
    them: an envelope line that is deleted turns a row of this file red).

What lies behind an input row is never zero: a tone of amplitude 1e3 behind fc32 rows, 0xEE (then 0x11) behind payload rows."""
import functools

import numpy as np
import pytest

import rows as R
from gain_cases import channel_estimate, same
from rows import Layout
from soft_ref import through_h
from util import assert_bytes_match, decision_margin, fc32, make_symbols_np, rel_err, through_channel, wide

pytestmark = pytest.mark.gpu
TOL = 1e-5
INVALID = -1
GIB = 1 << 30


def _api():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api

    return api


def _t(ctx, a, dtype):
    import torch

    return torch.tensor(np.asarray(a), dtype=dtype, device=ctx.device)


def _blank(ctx, n, dtype, value):
    import torch

    return torch.full((n,), value, dtype=dtype, device=ctx.device)


def _unaligned(lay):
    """a byte row that the dword-store kernels decline: (out | out_stride) & 3"""
    return (lay.base_off | lay.stride) & 3 != 0


# ================================================================================================================ rx_demod
DEMOD_SHAPES = [(64, 6, True, 12, 8), (64, 1, True, 5, 8), (512, 2, False, 5, 3), (4096, 8, True, 3, 2)]     # n, mod, guard, frames, symbols
HK_KINDS = ("none", "shared", "per frame")


@functools.lru_cache(maxsize=None)
def demod_case(orc, n, mod, guard, F, D):
    """F rows of D symbols at 34 dB as demod_pool draws them, per channel kind: the rows (through that channel), the channel as the GPU
    gets it, the oracle's bytes [F, r] and soft points [F, D * nd].  No oracle decision lies within 1e-4 of a boundary (asserted)."""
    rng = np.random.default_rng([6400, n, mod])
    x0, data = make_symbols_np(orc, rng, F * D, n, guard, mod, snr_db=34.0)
    x0 = x0.reshape(F, -1)
    hks = {"none": None, "shared": fc32(np.fft.fft(orc.channel_taps(), n)),
           "per frame": fc32(1.0 + 0.3 * (rng.standard_normal((F, n)) + 1j * rng.standard_normal((F, n))))}
    case = {"x": {}, "hk": hks, "bytes": {}, "soft": {}}
    for kind, hk in hks.items():
        x = x0 if hk is None else through_h(x0, n, hk.reshape(-1, n))
        by, soft = [], []
        for f in range(F):
            hf = None if hk is None else wide(hk.reshape(-1, n)[f if kind == "per frame" else 0])
            b, s = orc.rx_demod(wide(x[f]), n, guard, mod, hk=hf, want_soft=True)
            by.append(np.frombuffer(b, np.uint8)); soft.append(np.asarray(s))
        case["x"][kind], case["bytes"][kind], case["soft"][kind] = x, np.stack(by), np.stack(soft)
        assert decision_margin(case["soft"][kind], mod).min() >= 1e-4, (n, mod, kind)
    assert bytes(case["bytes"]["none"].ravel()) == data
    return case


def demod_expect(n, mod, guard, kind, lay, soft, F, D):
    """launch_demod64 / run_demod64_fast (kernels_n64.hip), run_demod_mid (kernels_mid.hip), run_demod4096 (kernels_n4096.hip)"""
    if soft or _unaligned(lay):
        return "k_sym<demod>"                              # (out | out_stride) & 3, or a soft output: the generic kernel
    if n == 4096:
        return "k_demod4096"
    if n != 64:
        return "k_demod_mid"
    if kind == "per frame" or D % 8:
        return "k_sym<demod>"                              # the N = 64 fast path takes a shared channel only
    region = (48 if guard else 64) * mod                   # bytes of an 8-symbol group
    wide_stores = region % 16 == 0 and lay.base_off % 16 == 0 and lay.stride % 16 == 0
    groups = F * D // 8
    burst = mod == 6 and guard and kind == "none" and wide_stores and groups % 4 == 0 and lay.stride == (D // 8) * region and lay.base_off % 128 == 0
    return "k_demod64" if not burst else "k_demod64<burst16>" if groups % 16 == 0 else "k_demod64<burst8>" if groups % 8 == 0 else "k_demod64<burst4>"


def demod_call(ctx, case, kind, n, F, D, out_lay, in_lay, soft=False):
    """one ofdm_rx_demod_batch -> (dispatch, bytes [F, r], soft [F, D * nd] or None), after the fill checks"""
    x = case["x"][kind]
    xflat, xptr = R.embed(ctx, x, in_lay, "tone")
    before = R.host_bytes(xflat)
    oflat, optr = R.embed(ctx, None, out_lay, "u8", n=F)
    hk = case["hk"][kind]
    hd = None if hk is None else ctx.to_device(hk)
    slay = Layout(0, case["soft"][kind].shape[1], case["soft"][kind].shape[1])
    sflat, sptr = R.embed(ctx, None, slay, "fc32", n=F) if soft else (None, None)
    rc = R.rx_demod(ctx, xptr, F, in_lay.stride, in_lay.row, 0, D, optr, out_lay.stride, hk=hd, hk_stride=n if kind == "per frame" else 0, soft=sptr)
    assert rc == 0, rc
    ctx.synchronize()
    disp = ctx.last_dispatch()
    assert R.only_rows_written(oflat, out_lay, F, "u8"), (disp, out_lay, in_lay)
    assert np.array_equal(R.host_bytes(xflat), before), (disp, in_lay)
    if soft:
        assert R.only_rows_written(sflat, slay, F, "fc32"), (disp, out_lay)
    return disp, R.read_rows(oflat, out_lay, F), (R.read_rows(sflat, slay, F) if soft else None)


@pytest.mark.parametrize("n,mod,guard,F,D", DEMOD_SHAPES)
def test_rx_demod_rows(orc, n, mod, guard, F, D):
    api = _api()
    case = demod_case(orc, n, mod, guard, F, D)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    S, r = ctx.S, D * ctx.bytes_per_symbol
    outs, ins = R.output_layouts(r), R.input_layouts(D * S)
    seen = set()
    for kind in HK_KINDS:
        want, wsoft = case["bytes"][kind], case["soft"][kind]
        disp, dense, _ = demod_call(ctx, case, kind, n, F, D, outs[0], ins[0])
        assert disp == demod_expect(n, mod, guard, kind, outs[0], False, F, D), (disp, kind)
        assert assert_bytes_match(bytes(dense.ravel()), bytes(want.ravel()), wsoft.ravel(), mod, what=f"dense {kind}") == 0
        for lay in outs[1:]:
            disp, got, _ = demod_call(ctx, case, kind, n, F, D, lay, ins[0])
            assert disp == demod_expect(n, mod, guard, kind, lay, False, F, D), (disp, kind, lay)
            assert np.array_equal(got, dense), (disp, kind, lay)
            seen.add(disp)
        for lay in ins[1:]:                                # frame_len = row < stride: the tone lies right behind every row
            disp, got, _ = demod_call(ctx, case, kind, n, F, D, outs[0], lay)
            assert disp == demod_expect(n, mod, guard, kind, outs[0], False, F, D), (disp, kind, lay)
            assert np.array_equal(got, dense), (disp, kind, lay)
        # soft_dev set: the generic kernel whatever the rows
        disp, got, dsoft = demod_call(ctx, case, kind, n, F, D, outs[0], ins[0], soft=True)
        assert disp == "k_sym<demod>" and np.array_equal(got, dense)
        assert rel_err(dsoft, wsoft) <= TOL, (kind, rel_err(dsoft, wsoft))
        for lay, il in ((outs[2], ins[1]), (outs[7], ins[2])):
            disp, got, soft = demod_call(ctx, case, kind, n, F, D, lay, il, soft=True)
            assert disp == "k_sym<demod>" and np.array_equal(got, dense) and same(soft, dsoft), (kind, lay)
    # one workgroup walks every row
    ctx.set_tuning("grid_cap", 1)
    for kind in ("none", "per frame"):
        dense = None
        for lay in (outs[0], outs[1], outs[3], outs[7]):
            disp, got, _ = demod_call(ctx, case, kind, n, F, D, lay, ins[1])
            assert disp == demod_expect(n, mod, guard, kind, lay, False, F, D), (disp, kind, lay)
            dense = got if dense is None else dense
            assert np.array_equal(got, dense) and bytes(got.ravel()) == bytes(case["bytes"][kind].ravel()), (kind, lay)
    if (n, mod) == (64, 6):                                # the names the envelope of launch_demod64 gives this shape, literally
        assert demod_expect(n, mod, guard, "none", outs[0], False, F, D) == "k_demod64<burst4>"
        assert [demod_expect(n, mod, guard, "none", lay, False, F, D) for lay in outs[1:]] == ["k_demod64"] * 4 + ["k_sym<demod>"] * 3
        assert demod_expect(n, mod, guard, "shared", outs[0], False, F, D) == "k_demod64"
    assert "k_sym<demod>" in seen and len(seen) >= 2


# ================================================================================================================ tx_encode
TX_SHAPES = [(64, 6, True, 300, 3), (64, 1, False, 37, 3), (256, 4, True, 700, 3), (4096, 8, True, 9000, 2)]   # n, mod, guard, payload bytes, frames
TX_FAST = {64: "k_txframe64", 256: "k_txframe_mid", 4096: "k_txframe4096"}
TX_GENERIC = "k_sym<tx>+k_tx_finish"


def tx_expect(n, out_lay):
    """run_txframe64 / run_txframe_mid / run_txframe4096 decline on out & 15 or an odd out_stride (in samples of 8 bytes)"""
    return TX_GENERIC if (out_lay.base_off * 8) % 16 or out_lay.stride % 2 else TX_FAST[n]


@functools.lru_cache(maxsize=None)
def tx_case(orc, n, mod, guard, nbytes, F):
    rng = np.random.default_rng([7000, n, mod])
    pay = rng.integers(0, 256, (F, nbytes), dtype=np.uint8)
    lens = rng.integers(1, nbytes, F).astype(np.int32)
    lens[0], lens[-1] = nbytes, 0                          # ragged lengths include payload_bytes and 0
    full = [orc.encode(bytes(pay[f]), guard, mod, n) for f in range(F)]
    ragged = [orc.encode(bytes(pay[f, :lens[f]]), guard, mod, n) for f in range(F)]
    return pay, lens, full, ragged


def tx_call(ctx, pay, lens, nbytes, pay_lay, out_lay, slack):
    """one ofdm_tx_encode_batch; the bytes behind a row's own length and behind payload_bytes are `slack` -> (dispatch, frames)"""
    F = pay.shape[0]
    rows = pay.copy()
    if lens is not None:
        for f in range(F):
            rows[f, lens[f]:] = slack
    pflat, pptr = R.embed(ctx, rows, pay_lay, slack)
    before = R.host_bytes(pflat)
    oflat, optr = R.embed(ctx, None, out_lay, "fc32", n=F)
    import torch

    ld = None if lens is None else _t(ctx, lens, torch.int32)
    rc = R.tx_encode(ctx, pptr, F, pay_lay.stride, ld, nbytes, optr, out_lay.stride)
    assert rc == 0, rc
    ctx.synchronize()
    disp = ctx.last_dispatch()
    assert R.only_rows_written(oflat, out_lay, F, "fc32"), (disp, out_lay, pay_lay)
    assert np.array_equal(R.host_bytes(pflat), before)
    return disp, R.read_rows(oflat, out_lay, F)


def assert_frames_are_the_oracles(frames, want, what):
    for f, w in enumerate(want):
        assert rel_err(frames[f, :w.size], w) <= TOL, (what, f, rel_err(frames[f, :w.size], w))


@pytest.mark.parametrize("n,mod,guard,nbytes,F", TX_SHAPES)
def test_tx_encode_rows(orc, n, mod, guard, nbytes, F):
    api = _api()
    pay, lens, full, ragged = tx_case(orc, n, mod, guard, nbytes, F)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    frame = ctx.frame_samples(nbytes)
    assert frame == full[0].size and frame % 2 == 0
    outs, pays = R.output_layouts(frame), R.payload_layouts(nbytes)
    for ln, want in ((None, full), (lens, ragged)):
        disp, dense = tx_call(ctx, pay, ln, nbytes, pays[0], outs[0], R.FILL_U8)
        assert disp == TX_FAST[n] == tx_expect(n, outs[0]), disp
        assert_frames_are_the_oracles(dense, want, "dense")
        generic = None
        for lay in outs[1:]:
            disp, got = tx_call(ctx, pay, ln, nbytes, pays[0], lay, R.FILL_U8)
            assert disp == tx_expect(n, lay), (disp, lay)
            if disp == TX_FAST[n]:
                assert same(got, dense), (disp, lay)
            else:                                          # an odd out_stride, or out % 16 == 8: the generic pair, held to the oracle
                assert_frames_are_the_oracles(got, want, lay)
                generic = got if generic is None else generic
                assert same(got, generic), (disp, lay)     # ... and to itself at every such layout
        assert [tx_expect(n, lay) for lay in outs[5:]] == [TX_GENERIC] * 3 and generic is not None
        for play in pays:
            for slack in (R.FILL_U8, R.FILL_U8_OTHER):     # what lies behind len_f and behind payload_bytes changes; the frames do not
                for lay, ref in ((outs[0], dense), (outs[6], generic)):
                    disp, got = tx_call(ctx, pay, ln, nbytes, play, lay, slack)
                    assert disp == tx_expect(n, lay), (disp, play, lay)
                    assert same(got, ref), (disp, play, slack, lay)
    ctx.set_tuning("grid_cap", 1)
    disp, got = tx_call(ctx, pay, lens, nbytes, pays[2], outs[2], R.FILL_U8_OTHER)
    assert disp == TX_FAST[n] and same(got, dense)


# ================================================================================================================ rx_decode
DECODE_SHAPES = [(64, 6, True, 560), (1024, 4, True, 1500), (256, 4, True, 300)]      # n, mod, guard, bytes of the frame's body
DECODE_SNR_DB = 40.0


def _decode_draw(orc, rng, n, mod, guard, nbytes, ecc, flen, span, delays, frame_lens, D):
    """one draw of the five captures -> (captures, {frame_len: the oracle's decodes}) or None when an oracle point that carries a
    delivered bit lies within 1e-4 of a boundary (the zero points transmit pads the last symbol with do not count: 0 is a boundary)"""
    S = n + n // 4
    caps = []
    for d in delays:
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        tx = orc.encode(orc.hamming74_encode(pay) if ecc else pay, guard, mod, n)
        assert tx.size == flen
        caps.append(through_channel(orc, rng, tx, span, d, (rng.random() * 1.6 - 0.8) * np.pi / S, DECODE_SNR_DB, data_start=10 * S))
    caps = np.stack(caps)
    want = {}
    for frame_len in frame_lens:
        ws = []
        for f in range(5):
            w = orc.decode_sc(wide(caps[f][:frame_len]), guard, mod, n, max_symbols=D, want_soft=True)
            assert w["status"] == 0, (n, ecc, frame_len, f)
            used = -(-(16 + len(w["bytes"])) * 8 // mod)
            if decision_margin(w["soft"][:used], mod).min() < 1e-4:
                return None
            w["payload"] = orc.hamming74_decode(w["bytes"])[0] if ecc else w["bytes"]
            ws.append(w)
        want[frame_len] = ws
    return caps, want


@functools.lru_cache(maxsize=None)
def decode_case(orc, n, mod, guard, body, ecc):
    """Five captures with the delays of frame_case (tests/test_gpu_llr_oracle.py) through the FIR channel at 40 dB; per frame_len (the
    slot, and half a symbol short of the latest frame's end, which cuts the late frames inside their last symbol) the oracle's decode of
    the capture cut there.  A symbol the capture cuts demodulates to points anywhere, so the captures are the first seeded draw whose
    oracle points keep 1e-4 from every boundary: a condition on the inputs, after which every kernel owes the oracle's bytes exactly."""
    S = n + n // 4
    nbytes = body // 7 * 4 if ecc else body                # Hamming(7,4): the coded body has the same size
    flen = orc.frame_len(len(orc.hamming74_encode(bytes(nbytes))) if ecc else nbytes, n, guard, mod)
    D = flen // S - 10
    span = 2176 if n == 64 else flen + 2 * S
    delays = [3, S // 4, 17, S // 2 + S // 4, S - 5]
    assert max(delays) + flen <= span
    for draw in range(32):
        got = _decode_draw(orc, np.random.default_rng([7100, n, ecc, draw]), n, mod, guard, nbytes, ecc, flen, span, delays,
                           (span, max(delays) + flen - S // 2), D)
        if got is not None:
            return got[0], D, got[1]
    raise AssertionError("no draw keeps the oracle's points off the boundaries")


def decode_expect(n, ecc, out_lay, frame_len, D):
    """rx_front_end + rx_decode_inner (ofdm_abi.hip), run_rxframe64 (kernels_n64.hip), run_rxframe1024 (kernels_rx1024.hip)"""
    odd = _unaligned(out_lay)
    if n == 64:
        roomy = frame_len >= (10 + D) * 80 + 64            # room for the longest frame and a 64-sample start: the cut frames get a launch of their own
        fin = ecc == 0 and not odd                         # to_final: the payload goes straight to 4-byte aligned rows
        return "k_sc80+k_sc_tile<list>+k_rx_prepare+" + ("k_rxframe64<finish>" if fin else "k_rxframe64") + \
               ("+k_rxframe64<cut,list>" if roomy else "") + ("" if fin else "+k_rx_finish")
    if n == 1024:                                          # the raw rows (4 symbols of 384 bytes) fit the LDS image: fused unless the rows are unaligned
        return "k_sc_stream<regs>+k_rx_prepare+" + ("k_rxframe1024+k_rx_finish" if odd else "k_rxframe1024<finish>")
    return "k_sc_stream+k_rx_prepare+k_sym<chest>+k_demod_mid<frame>+k_rx_finish"


def decode_call(ctx, caps, frame_len, D, in_lay, out_lay):
    import torch

    F = caps.shape[0]
    x = caps.copy()
    x[:, frame_len:] = R.fill_buffer("tone", caps.shape[1] - frame_len)       # loud behind frame_len, inside the row
    xflat, xptr = R.embed(ctx, x, in_lay, "tone")
    before = R.host_bytes(xflat)
    oflat, optr = R.embed(ctx, None, out_lay, "u8", n=F)
    res = {"len": _blank(ctx, F, torch.int32, -77), "status": _blank(ctx, F, torch.int32, -77), "offset": _blank(ctx, F, torch.int32, -77),
           "f_delta": _blank(ctx, F, torch.float64, -77.0), "metric": _blank(ctx, F, torch.float32, -77.0)}
    rc = R.rx_decode(ctx, xptr, F, in_lay.stride, frame_len, 0, D, optr, out_lay.stride, res["len"], res["status"], res["offset"],
                     res["f_delta"], res["metric"])
    assert rc == 0, rc
    ctx.synchronize()
    disp = ctx.last_dispatch()
    assert R.only_rows_written(oflat, out_lay, F, "u8"), (disp, out_lay, in_lay)
    assert np.array_equal(R.host_bytes(xflat), before), (disp, in_lay)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res["bytes"] = R.read_rows(oflat, out_lay, F)
    return disp, res


def assert_same_decode(got, dense, what):
    for k in ("len", "status", "offset", "f_delta", "metric"):
        assert same(got[k], dense[k]), (what, k, got[k], dense[k])
    for f, ln in enumerate(dense["len"]):
        assert np.array_equal(got["bytes"][f, :ln], dense["bytes"][f, :ln]), (what, f)


@pytest.mark.parametrize("ecc", [0, 1])
@pytest.mark.parametrize("n,mod,guard,body", DECODE_SHAPES)
def test_rx_decode_rows(orc, n, mod, guard, body, ecc):
    api = _api()
    caps, D, want = decode_case(orc, n, mod, guard, body, ecc)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc)
    r = ctx.decode_row_bytes(D)
    outs, ins = R.output_layouts(r), R.input_layouts(caps.shape[1])
    names = set()
    for frame_len, ws in want.items():
        disp, dense = decode_call(ctx, caps, frame_len, D, ins[0], outs[0])
        assert disp == decode_expect(n, ecc, outs[0], frame_len, D), (disp, frame_len)
        for f, w in enumerate(ws):
            assert dense["status"][f] == 0 and dense["offset"][f] == w["offset"] and abs(dense["f_delta"][f] - w["f_delta"]) <= 1e-9, (frame_len, f)
            assert abs(dense["metric"][f] - w["metric"]) <= 1e-6 * max(1.0, w["metric"]), (frame_len, f)
            assert dense["len"][f] == len(w["payload"]) and bytes(dense["bytes"][f, :dense["len"][f]]) == w["payload"], (frame_len, f)
        for lay in outs[1:]:
            disp, got = decode_call(ctx, caps, frame_len, D, ins[0], lay)
            assert disp == decode_expect(n, ecc, lay, frame_len, D), (disp, lay, frame_len)
            assert_same_decode(got, dense, (lay, frame_len))
            names.add(disp)
        for il, lay in ((ins[1], outs[0]), (ins[2], outs[0]), (ins[1], outs[7]), (ins[2], outs[2])):
            disp, got = decode_call(ctx, caps, frame_len, D, il, lay)
            assert disp == decode_expect(n, ecc, lay, frame_len, D), (disp, il, lay, frame_len)
            assert_same_decode(got, dense, (il, lay, frame_len))
    assert min(want) < max(w["offset"] for w in want[min(want)]) + (10 + D) * ctx.S          # the short frame_len cuts the latest frame
    if n == 64:
        # tight rows of odd length (stride == frame_len): k_sc80 reads in 16-byte units, so ofdm_abi_sc_run peels the last row off and
        # sends it through the general search on its own; its CFO and metric are that detector's, held to the oracle
        frame_len = min(want)
        assert frame_len % 2 == 1
        disp, got = decode_call(ctx, caps[:, :frame_len], frame_len, D, Layout(0, frame_len, frame_len), outs[0])
        assert disp == decode_expect(n, ecc, outs[0], frame_len, D).replace("+k_rx_prepare", "+k_sc_tile+k_rx_prepare"), disp
        w = want[frame_len][-1]
        assert abs(got["f_delta"][-1] - w["f_delta"]) <= 1e-9 and abs(got["metric"][-1] - w["metric"]) <= 1e-6 * max(1.0, w["metric"])
        got["f_delta"][-1], got["metric"][-1] = dense["f_delta"][-1], dense["metric"][-1]
        assert_same_decode(got, dense, "tight odd rows")
    if n == 1024:                                          # unaligned rows move the finish out of the frame kernel
        assert {d.split("k_rx_prepare+")[1] for d in names} == {"k_rxframe1024<finish>", "k_rxframe1024+k_rx_finish"}
    if n == 64 and not ecc:
        assert {d.split("k_rx_prepare+")[1].split("+")[0] for d in names} == {"k_rxframe64<finish>", "k_rxframe64"}


def test_rx_decode_1024_raw_rows_beyond_the_lds_image(orc):
    """run_rxframe1024 fuses the finish only while the RAW row (max_symbols * bytes_per_symbol, rounded up to dwords) fits its LDS
    image of RX_RAW_DW * 4 = 3584 bytes: that bound is on max_symbols, not on the caller's out_stride.  The frames of the N = 1024
    case (4 symbols of 384 bytes) decoded with max_symbols = 10 (3840 bytes): k_rxframe1024 + k_rx_finish, the same payloads."""
    api = _api()
    caps, D, want = decode_case(orc, 1024, 4, True, 1500, 0)
    ctx = api.Context(n_fft=1024, modulation=4, guard_bands=True)
    assert D * ctx.bytes_per_symbol <= 3584 < 10 * ctx.bytes_per_symbol
    span = caps.shape[1]
    _, dense = decode_call(ctx, caps, span, D, Layout(0, span, span), R.output_layouts(ctx.decode_row_bytes(D))[0])
    for lay in (R.output_layouts(ctx.decode_row_bytes(10))[i] for i in (0, 2, 7)):
        disp, got = decode_call(ctx, caps, span, 10, Layout(0, span + 7, span), lay)
        assert disp == "k_sc_stream<regs>+k_rx_prepare+k_rxframe1024+k_rx_finish", disp
        assert_same_decode(got, dense, lay)


# ================================================================================================================ small stages
STAGE_SHAPES = [(64, 1120), (1024, 2560)]                 # n, samples per row (N = 1024: two 2048-sample chunks of k_frame_max)


def _inplace(ctx, x, lay, call):
    """an in-place stage on rows x in layout lay -> the rows afterwards; the slack must leave bit for bit as it came"""
    flat, ptr = R.embed(ctx, x, lay, "tone")
    assert call(ptr, lay.stride) == 0
    ctx.synchronize()
    assert ctx.last_dispatch() == ""                       # k_frame_max / k_frame_scale / k_cfo_rotate: one form each, nothing traced
    assert R.only_rows_written(flat, lay, x.shape[0], "tone"), lay
    return R.read_rows(flat, lay, x.shape[0])


@pytest.mark.parametrize("n,ln", STAGE_SHAPES)
def test_normalize_and_cfo_rotate_on_padded_rows(orc, n, ln):
    import torch

    api = _api()
    rng = np.random.default_rng(7200 + n)
    ctx = api.Context(n_fft=n, modulation=4)
    F = 4
    x = fc32(rng.standard_normal((F, ln)) + 1j * rng.standard_normal((F, ln)))
    x[1] *= 1e-3                                           # a quiet row next to loud slack
    x[2, -1] = 9.0 + 0j                                    # the maximum is the row's last sample
    x[3, 0] = 0 + 7.5j                                     # ... its first, in the imaginary part
    lays = R.input_layouts(ln) + [Layout(3, ln + 64, ln)]
    dense = _inplace(ctx, x, lays[0], lambda p, s: R.normalize(ctx, p, F, s, ln))
    for f in range(F):
        assert rel_err(dense[f], orc.normalize(wide(x[f]))) <= TOL, f
        assert abs(max(dense[f].real.max(), dense[f].imag.max()) - 1.0) < 1e-6
    for lay in lays[1:]:
        assert same(_inplace(ctx, x, lay, lambda p, s: R.normalize(ctx, p, F, s, ln)), dense), lay
    # frame_len below the row: the row's own tail is slack too
    cut = ln - 37
    xt = x.copy()
    xt[:, cut:] = R.fill_buffer("tone", 37)
    got = _inplace(ctx, xt, lays[1], lambda p, s: R.normalize(ctx, p, F, s, cut))
    assert same(got[:, cut:], xt[:, cut:])
    for f in range(F):
        assert rel_err(got[f, :cut], orc.normalize(wide(x[f, :cut]))) <= TOL, f
    fds = np.array([0.0371, -0.0123, 0.0, 2.1e-3])
    first = np.array([0, 777, 5, 3], np.int32)
    fd_d, fi_d = _t(ctx, fds, torch.float64), _t(ctx, first, torch.int32)
    dense = _inplace(ctx, x, lays[0], lambda p, s: R.cfo_rotate(ctx, p, F, s, ln, fd_d, fi_d))
    for f in range(F):
        assert rel_err(dense[f], orc.cfo_rotate(wide(x[f]), float(fds[f]), int(first[f]))) <= TOL, f
    for lay in lays[1:]:
        assert same(_inplace(ctx, x, lay, lambda p, s: R.cfo_rotate(ctx, p, F, s, ln, fd_d, fi_d)), dense), lay
    # a stride below the row: refused, nothing written
    flat, ptr = R.embed(ctx, x, lays[0], "tone")
    before = R.host_bytes(flat)
    assert R.normalize(ctx, ptr, F, ln - 1, ln) == INVALID
    ctx.synchronize()
    assert np.array_equal(R.host_bytes(flat), before)


@pytest.mark.parametrize("n,mod,nbytes", [(64, 2, 100), (1024, 4, 300)])
def test_estimate_channel_rows(orc, n, mod, nbytes):
    import torch

    api = _api()
    rng = np.random.default_rng(7300 + n)
    ctx = api.Context(n_fft=n, modulation=mod)
    S, F = ctx.S, 4
    span = ctx.frame_samples(nbytes) + S
    caps, offs, fds = [], [], []
    for f in range(F):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), False, mod, n)
        d, fd = int(rng.integers(0, S // 2)), float((rng.random() - 0.5) * 2.0 / S)
        caps.append(through_channel(orc, rng, tx, span, d, fd, 30.0, data_start=10 * S)); offs.append(d + 5); fds.append(fd)
    caps = np.stack(caps)
    od, fdd = _t(ctx, offs, torch.int32), _t(ctx, fds, torch.float64)
    trn = orc.default_training(n)
    hlay = Layout(0, n, n)
    dense = None
    for lay in R.input_layouts(span):
        xflat, xptr = R.embed(ctx, caps, lay, "tone")
        before = R.host_bytes(xflat)
        hflat, hptr = R.embed(ctx, None, hlay, "fc32", n=F)
        assert R.estimate_channel(ctx, xptr, F, lay.stride, span, od, fdd, hptr) == 0
        ctx.synchronize()
        assert ctx.last_dispatch() == "k_sym<chest>"
        assert R.only_rows_written(hflat, hlay, F, "fc32") and np.array_equal(R.host_bytes(xflat), before)
        hk = R.read_rows(hflat, hlay, F)
        if dense is None:
            dense = hk
            for f in range(F):
                assert rel_err(hk[f], channel_estimate(orc, wide(caps[f]), offs[f], fds[f], trn, n)) <= TOL, f
        assert same(hk, dense), lay


@pytest.mark.parametrize("n,a_len", [(64, 333), (1024, 3000)])
def test_xcorr_rows(orc, n, a_len):
    import torch

    api = _api()
    rng = np.random.default_rng(7400 + n)
    ctx = api.Context(n_fft=n)
    F, nb = 4, n + n // 4
    lock = fc32(orc.locking_signal(nb))
    a = fc32(0.05 * (rng.standard_normal((F, a_len)) + 1j * rng.standard_normal((F, a_len))))
    for f in range(F):
        a[f, 11 * f + 3: 11 * f + 3 + nb] += lock
    bd = ctx.to_device(lock)
    r = 2 * a_len - 1
    dense = None
    for il, ol in zip(R.input_layouts(a_len) + [Layout(0, a_len + 64, a_len)], [Layout(0, r, r), Layout(0, r + 16, r), Layout(1, r + 1, r), Layout(3, r + 5, r)]):
        aflat, aptr = R.embed(ctx, a, il, "tone")
        before = R.host_bytes(aflat)
        oflat, optr = R.embed(ctx, None, ol, "fc32", n=F)
        idx, pk = _blank(ctx, F, torch.int32, -77), _blank(ctx, F, torch.float32, -77.0)
        assert R.xcorr(ctx, aptr, F, il.stride, a_len, bd, nb, idx, pk, optr, ol.stride) == 0
        ctx.synchronize()
        assert ctx.last_dispatch() == ""                   # k_xcorr: one form, nothing traced
        assert R.only_rows_written(oflat, ol, F, "fc32"), (il, ol)
        assert np.array_equal(R.host_bytes(aflat), before)
        got = (idx.cpu().numpy(), pk.cpu().numpy(), R.read_rows(oflat, ol, F))
        if dense is None:
            dense = got
            for f in range(F):
                wi, wout = orc.xcorr_fft(wide(a[f]), wide(lock))
                assert got[0][f] == wi == 11 * f + 3 + a_len - 1 and rel_err(got[2][f], wout) <= TOL, f
                assert abs(float(got[1][f]) - abs(wout[wi])) <= 1e-5 * abs(wout[wi])
        assert all(same(g, d) for g, d in zip(got, dense)), (il, ol)
    oflat, optr = R.embed(ctx, None, Layout(0, r, r), "fc32", n=F)
    assert R.xcorr(ctx, aptr, F, il.stride, a_len, bd, nb, idx, pk, optr, r - 1) == INVALID
    ctx.synchronize()
    assert R.only_rows_written(oflat, Layout(0, r, r), F, "fc32", lens=[0] * F)


@pytest.mark.parametrize("n", [64, 1024])
def test_frequency_correction_rows(orc, n):
    import torch

    api = _api()
    rng = np.random.default_rng(7500 + n)
    ctx = api.Context(n_fft=n)
    S, F = ctx.S, 4
    left = fc32(rng.standard_normal((F, S)) + 1j * rng.standard_normal((F, S)))
    fds = rng.random(F) * 2.0 / S
    right = fc32(left * np.exp(1j * fds[:, None] * S) + 0.01 * (rng.standard_normal((F, S)) + 1j * rng.standard_normal((F, S))))
    want = [orc.frequency_correction(wide(left[f]), wide(right[f])) for f in range(F)]
    dense = None
    for base, gap, pad in ((0, 0, 0), (1, 0, 1), (0, 3, 4), (3, S // 2 + 1, 6)):      # right_offset = S + gap, stride = 2 S + gap + pad
        row = np.concatenate([left, R.fill_buffer("tone", F * gap).reshape(F, gap), right], axis=1)
        lay = Layout(base, row.shape[1] + pad, row.shape[1])
        flat, ptr = R.embed(ctx, row, lay, "tone")
        before = R.host_bytes(flat)
        out = _blank(ctx, F + 2, torch.float64, -77.0)
        assert R.frequency_correction(ctx, ptr, F, lay.stride, S + gap, out) == 0
        ctx.synchronize()
        assert ctx.last_dispatch() == ""                   # k_freq_corr: one form, nothing traced
        got = out.cpu().numpy()
        assert np.array_equal(R.host_bytes(flat), before) and (got[F:] == -77.0).all()
        if dense is None:
            dense = got
            assert all(abs(got[f] - want[f]) <= 1e-12 for f in range(F)), (got, want)
        assert same(got, dense), (base, gap, pad)


# ================================================================================================================ host forms
def _host_buffer(api, nbytes, pinned):
    return api.pinned_empty((nbytes,), np.uint8) if pinned else np.empty(nbytes, np.uint8)


def _host_embed(api, rows, lay, fill, pinned, n=None):
    """R.embed in host memory, pageable or page-locked -> (flat, address of row 0)"""
    proto, _ = R.embed(None, rows, lay, fill, n=n)
    raw = _host_buffer(api, proto.nbytes + 128, pinned)
    skip = (-raw.ctypes.data) % 128
    flat = raw[skip: skip + proto.nbytes].view(proto.dtype)
    flat[:] = proto
    return flat, flat.ctypes.data + lay.base_off * flat.dtype.itemsize, raw


@pytest.mark.parametrize("pinned", [False, True])
def test_rx_demod_host_scatters_into_padded_rows(orc, pinned):
    api = _api()
    n, mod, guard, F, D = DEMOD_SHAPES[0]
    case = demod_case(orc, n, mod, guard, F, D)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    r, ln = D * ctx.bytes_per_symbol, D * ctx.S
    _, dev_bytes, _ = demod_call(ctx, case, "none", n, F, D, R.output_layouts(r)[0], R.input_layouts(ln)[0])
    assert bytes(dev_bytes.ravel()) == bytes(case["bytes"]["none"].ravel())
    for chunk in (0, 2):
        for il, ol in ((Layout(0, ln, ln), Layout(0, r, r)), (Layout(0, ln + 7, ln), Layout(0, r + 16, r)), (Layout(1, ln + 1, ln), Layout(3, r + 5, r))):
            xflat, xptr, _x = _host_embed(api, case["x"]["none"], il, "tone", pinned)
            before = xflat.copy()
            oflat, optr, _o = _host_embed(api, None, ol, "u8", pinned, n=F)
            if pinned:
                assert ctx.lib.ofdm_host_is_pinned(xptr, 8) == 1 and ctx.lib.ofdm_host_is_pinned(optr, 1) == 1
            assert R.rx_demod_host(ctx, xptr, F, il.stride, ln, 0, D, optr, ol.stride, chunk) == 0
            groups = (2 if chunk else F) * D // 8          # the library's own staging rows are dense and aligned: the shape picks the burst
            assert ctx.last_dispatch() == ("k_demod64<burst4>" if groups % 4 == 0 else "k_demod64"), (ctx.last_dispatch(), chunk)
            assert R.only_rows_written(oflat, ol, F, "u8"), (chunk, il, ol)
            assert same(xflat, before)
            assert np.array_equal(R.read_rows(oflat, ol, F), dev_bytes), (chunk, il, ol)
    oflat, optr, _o = _host_embed(api, None, Layout(0, r, r), "u8", pinned, n=F)
    assert R.rx_demod_host(ctx, xptr, F, il.stride, ln, 0, D, optr, r - 1, 0) == INVALID
    assert R.rx_demod_host(ctx, xptr, F, ln - 1, ln, 0, D, optr, r, 0) == INVALID
    assert R.only_rows_written(oflat, Layout(0, r, r), F, "u8", lens=[0] * F)


@pytest.mark.parametrize("pinned", [False, True])
def test_rx_decode_host_scatters_into_padded_rows(orc, pinned):
    api = _api()
    n, mod, guard, body = DECODE_SHAPES[0]
    caps, D, want = decode_case(orc, n, mod, guard, body, 0)
    caps = caps[:4]                                        # chunks of 2 frames: no chunk is a single row (an odd frame_len needs slack behind the row for k_sc80)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    F, span = caps.shape
    r = ctx.decode_row_bytes(D)
    frame_len = min(want)                                  # the tone lies behind frame_len inside the row and behind the row
    assert frame_len % 2 == 1 and max(w["offset"] for w in want[frame_len][:4]) + (10 + D) * ctx.S > frame_len
    x = caps.copy()
    x[:, frame_len:] = R.fill_buffer("tone", span - frame_len)
    _, dense = decode_call(ctx, caps, frame_len, D, Layout(0, span, span), R.output_layouts(r)[0])
    for chunk in (0, 2):
        for il, ol in ((Layout(0, span, span), Layout(0, r, r)), (Layout(0, span + 7, span), Layout(0, r + 16, r)), (Layout(1, span + 1, span), Layout(3, r + 5, r))):
            xflat, xptr, _x = _host_embed(api, x, il, "tone", pinned)
            before = xflat.copy()
            oflat, optr, _o = _host_embed(api, None, ol, "u8", pinned, n=F)
            res = {"len": np.full(F, -77, np.int32), "status": np.full(F, -77, np.int32), "offset": np.full(F, -77, np.int32),
                   "f_delta": np.full(F, -77.0), "metric": np.full(F, -77.0, np.float32)}
            rc = R.rx_decode_host(ctx, xptr, F, il.stride, frame_len, 0, D, optr, ol.stride, res["len"], res["status"], res["offset"],
                                  res["f_delta"], res["metric"], chunk)
            assert rc == 0, rc
            assert ctx.last_dispatch() == decode_expect(n, 0, Layout(0, r, r), frame_len, D), ctx.last_dispatch()    # the staging rows are the library's own
            assert R.only_rows_written(oflat, ol, F, "u8"), (chunk, il, ol)
            assert same(xflat, before)
            res["bytes"] = R.read_rows(oflat, ol, F)
            assert_same_decode(res, dense, (chunk, il, ol))
    oflat, optr, _o = _host_embed(api, None, Layout(0, r, r), "u8", pinned, n=F)
    args = (res["len"], res["status"], res["offset"], res["f_delta"], res["metric"], 0)
    assert R.rx_decode_host(ctx, xptr, F, il.stride, frame_len, 0, D, optr, r - 1, *args) == INVALID
    assert R.rx_decode_host(ctx, xptr, F, frame_len - 1, frame_len, 0, D, optr, r, *args) == INVALID
    assert R.only_rows_written(oflat, Layout(0, r, r), F, "u8", lens=[0] * F)


# ================================================================================================================ refusals
def test_a_stride_below_the_row_is_refused_and_writes_nothing(orc):
    import torch

    api = _api()
    n, mod, guard, F, D = DEMOD_SHAPES[0]
    case = demod_case(orc, n, mod, guard, F, D)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    r, ln = D * ctx.bytes_per_symbol, D * ctx.S
    xd = ctx.to_device(case["x"]["none"])
    lay = Layout(0, r, r)
    oflat, optr = R.embed(ctx, None, lay, "u8", n=F)
    assert R.rx_demod(ctx, xd, F, ln, ln, 0, D, optr, r - 1) == INVALID
    res = [_blank(ctx, F, torch.int32, -77) for _ in range(2)]
    rd = ctx.decode_row_bytes(D)
    assert rd <= r
    assert R.rx_decode(ctx, xd, F, ln, ln, 0, D, optr, rd - 1, res[0], res[1]) == INVALID
    ctx.synchronize()
    assert R.only_rows_written(oflat, lay, F, "u8", lens=[0] * F) and all(bool((t == -77).all()) for t in res)
    # transmit: rows shorter than the frame; payload rows that overlap
    nbytes = 300
    frame = ctx.frame_samples(nbytes)
    pd = ctx.to_device(np.zeros((3, nbytes), np.uint8))
    flay = Layout(0, frame, frame)
    fflat, fptr = R.embed(ctx, None, flay, "fc32", n=3)
    assert R.tx_encode(ctx, pd, 3, nbytes, None, nbytes, fptr, frame - 1) == INVALID
    assert R.tx_encode(ctx, pd, 3, nbytes - 1, None, nbytes, fptr, frame) == INVALID
    ctx.synchronize()
    assert R.only_rows_written(fflat, flay, 3, "fc32", lens=[0] * 3)


# ================================================================================================================ rows far apart
FAR_SAMPLES = (1 << 31) + 8           # fc32 row stride: 16 GiB + 64 bytes; row 1 starts beyond 2^31 samples, 2^31 and 2^32 bytes
FAR_BYTES = (1 << 32) + 48            # byte row stride
WINDOW = 1 << 20                      # bytes of fill checked on either side of each row


class Far:
    """Two rows `stride` elements apart in one allocation that is never touched as a whole: torch.empty, the fill written to a WINDOW on
    either side of each row only, and checked there."""

    def __init__(self, ctx, rows, row, stride, fill, dtype):
        import torch

        free, _ = torch.cuda.mem_get_info(ctx.device)
        if free < 24 * GIB:
            pytest.skip(f"torch.cuda.mem_get_info() reports {free / GIB:.1f} GiB free, below the 24 GiB the rows 16 GiB apart need")
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.win = WINDOW // self.item
        self.row, self.stride, self.fill = row, stride, fill
        self.lay = Layout(self.win, stride, row)
        total = self.win + stride + row + self.win
        assert total * self.item < 18 * GIB
        self.flat = torch.empty(total, dtype=dtype, device=ctx.device)
        assert self.flat.data_ptr() % 128 == 0
        self.pattern = torch.from_numpy(R.fill_buffer(fill, 2 * self.win + row).view(np.uint8)).to(ctx.device).view(dtype)
        for f in range(2):
            s = self.lay.start(f)
            self.flat[s - self.win: s + row + self.win] = self.pattern
            if rows is not None:
                self.flat[s: s + row] = torch.from_numpy(np.ascontiguousarray(rows[f])).to(ctx.device)
        self.ptr = self.flat.data_ptr() + self.win * self.item
        assert self.lay.start(1) * self.item > 1 << 32 and (self.item == 1 or self.lay.start(1) > 1 << 31)

    def rows(self):
        return np.stack([self.flat[self.lay.start(f): self.lay.start(f) + self.row].cpu().numpy() for f in range(2)])

    def windows_hold_the_fill(self):
        import torch

        p = self.pattern.view(torch.uint8)
        w, rb = self.win * self.item, self.row * self.item
        for f in range(2):
            s = self.lay.start(f)
            got = self.flat[s - self.win: s + self.row + self.win].view(torch.uint8)
            if not (torch.equal(got[:w], p[:w]) and torch.equal(got[w + rb:], p[w + rb:])):
                return False
        return True

    def rows_hold(self, rows):
        return all(same(self.flat[self.lay.start(f): self.lay.start(f) + self.row], np.ascontiguousarray(rows[f])) for f in range(2))


def _release():
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("far", ["in", "out"])
@pytest.mark.parametrize("n,mod,guard,D", [(64, 6, True, 8), (4096, 8, True, 2)])
def test_rx_demod_rows_far_apart(orc, n, mod, guard, D, far):
    import torch

    api = _api()
    F = 2
    case = demod_case(orc, n, mod, guard, *[s for s in DEMOD_SHAPES if s[0] == n and s[1] == mod][0][3:])
    x, want = case["x"]["none"][:F], case["bytes"]["none"][:F]
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    r, ln = D * ctx.bytes_per_symbol, D * ctx.S
    fast = "k_demod64" if n == 64 else "k_demod4096"      # two groups: no burst
    buf = None
    try:
        if far == "in":
            buf = Far(ctx, x, ln, FAR_SAMPLES, "tone", torch.complex64)
            oflat, optr = R.embed(ctx, None, Layout(0, r, r), "u8", n=F)
            assert R.rx_demod(ctx, buf.ptr, F, FAR_SAMPLES, ln, 0, D, optr, r) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == fast
            got = R.read_rows(oflat, Layout(0, r, r), F)
            assert R.only_rows_written(oflat, Layout(0, r, r), F, "u8") and buf.windows_hold_the_fill() and buf.rows_hold(x)
        else:
            buf = Far(ctx, None, r, FAR_BYTES, "u8", torch.uint8)
            assert R.rx_demod(ctx, ctx.to_device(x), F, ln, ln, 0, D, buf.ptr, FAR_BYTES) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == fast
            got = buf.rows()
            assert buf.windows_hold_the_fill()
        assert np.array_equal(got, want)                   # the dense call's bytes are the oracle's (test_rx_demod_rows)
    finally:
        buf = None
        _release()


@pytest.mark.parametrize("far", ["payload", "out"])
@pytest.mark.parametrize("n,mod,guard,nbytes", [s[:4] for s in TX_SHAPES if s[0] in (64, 4096) and s[1] != 1])
def test_tx_encode_rows_far_apart(orc, n, mod, guard, nbytes, far):
    import torch

    api = _api()
    F = 2
    pay, _, full, _ = tx_case(orc, n, mod, guard, nbytes, [s for s in TX_SHAPES if s[0] == n and s[1] == mod][0][4])
    pay = pay[:F]
    lens = np.array([nbytes, nbytes // 3], np.int32)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    frame = ctx.frame_samples(nbytes)
    _, dense = tx_call(ctx, pay, lens, nbytes, Layout(0, nbytes, nbytes), Layout(0, frame, frame), R.FILL_U8)
    assert rel_err(dense[0], full[0]) <= TOL
    rows = pay.copy()
    rows[1, lens[1]:] = R.FILL_U8
    ld = _t(ctx, lens, torch.int32)
    buf = None
    try:
        if far == "payload":
            buf = Far(ctx, rows, nbytes, FAR_BYTES, "u8", torch.uint8)
            flay = Layout(0, frame, frame)
            oflat, optr = R.embed(ctx, None, flay, "fc32", n=F)
            assert R.tx_encode(ctx, buf.ptr, F, FAR_BYTES, ld, nbytes, optr, frame) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == TX_FAST[n]
            got = R.read_rows(oflat, flay, F)
            assert R.only_rows_written(oflat, flay, F, "fc32") and buf.windows_hold_the_fill() and buf.rows_hold(rows)
        else:
            buf = Far(ctx, None, frame, FAR_SAMPLES, "fc32", torch.complex64)
            assert R.tx_encode(ctx, ctx.to_device(rows), F, nbytes, ld, nbytes, buf.ptr, FAR_SAMPLES) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == TX_FAST[n]
            got = buf.rows()
            assert buf.windows_hold_the_fill()
        assert same(got, dense)
    finally:
        buf = None
        _release()


@pytest.mark.parametrize("far", ["in", "out"])
def test_rx_decode_rows_far_apart(orc, far):
    """k_sc80 takes row strides up to 2^27 samples (sc80_ok) and the filter pair even frame lengths only (sc_fast_ok): captures 2^31 + 8
    samples apart with an odd frame_len go through k_sc_tile, so their CFO and metric are held to the oracle, everything else to the
    dense call."""
    import torch

    api = _api()
    n, mod, guard, body = DECODE_SHAPES[0]
    caps, D, want = decode_case(orc, n, mod, guard, body, 0)
    caps, F = caps[3:5], 2                                 # the two latest frames
    span = caps.shape[1]
    frame_len = min(want)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    r = ctx.decode_row_bytes(D)
    disp0, dense = decode_call(ctx, caps, frame_len, D, Layout(0, span, span), Layout(0, r, r))
    assert disp0 == decode_expect(n, 0, Layout(0, r, r), frame_len, D)
    for f in range(F):
        w = want[frame_len][3 + f]
        assert dense["offset"][f] == w["offset"] and bytes(dense["bytes"][f, :dense["len"][f]]) == w["payload"]
    x = caps.copy()
    x[:, frame_len:] = R.fill_buffer("tone", span - frame_len)
    res = {"len": _blank(ctx, F, torch.int32, -77), "status": _blank(ctx, F, torch.int32, -77), "offset": _blank(ctx, F, torch.int32, -77),
           "f_delta": _blank(ctx, F, torch.float64, -77.0), "metric": _blank(ctx, F, torch.float32, -77.0)}
    tail = (res["len"], res["status"], res["offset"], res["f_delta"], res["metric"])
    buf = None
    try:
        if far == "in":
            buf = Far(ctx, x, span, FAR_SAMPLES, "tone", torch.complex64)
            oflat, optr = R.embed(ctx, None, Layout(0, r, r), "u8", n=F)
            assert R.rx_decode(ctx, buf.ptr, F, FAR_SAMPLES, frame_len, 0, D, optr, r, *tail) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == "k_sc_tile+k_rx_prepare+k_rxframe64<finish>", ctx.last_dispatch()
            got = R.read_rows(oflat, Layout(0, r, r), F)
            assert R.only_rows_written(oflat, Layout(0, r, r), F, "u8") and buf.windows_hold_the_fill() and buf.rows_hold(x)
        else:
            buf = Far(ctx, None, r, FAR_BYTES, "u8", torch.uint8)
            assert R.rx_decode(ctx, ctx.to_device(x), F, span, frame_len, 0, D, buf.ptr, FAR_BYTES, *tail) == 0
            ctx.synchronize()
            assert ctx.last_dispatch() == disp0
            got = buf.rows()
            assert buf.windows_hold_the_fill()
        out = {k: v.cpu().numpy() for k, v in res.items()}
        out["bytes"] = got
        if far == "in":                                    # another detector: its floats against the oracle, by the existing bars
            for f in range(F):
                w = want[frame_len][3 + f]
                assert abs(out["f_delta"][f] - w["f_delta"]) <= 1e-9 and abs(out["metric"][f] - w["metric"]) <= 1e-6 * max(1.0, w["metric"]), f
            out["f_delta"], out["metric"] = dense["f_delta"], dense["metric"]
        assert_same_decode(out, dense, far)
    finally:
        buf = None
        _release()


@pytest.mark.parametrize("n", [64, 4096])
def test_estimate_channel_and_normalize_rows_far_apart(orc, n):
    import torch

    api = _api()
    rng = np.random.default_rng(7600 + n)
    ctx = api.Context(n_fft=n, modulation=4)
    S, F = ctx.S, 2
    span = 11 * S
    caps, offs, fds = [], [], []
    for f in range(F):
        tx = orc.encode(bytes(rng.integers(0, 256, 20, dtype=np.uint8)), False, 4, n)
        d, fd = 7 + 20 * f, float((rng.random() - 0.5) * 2.0 / S)
        caps.append(through_channel(orc, rng, tx, span, d, fd, 30.0, data_start=10 * S)); offs.append(d + 5); fds.append(fd)
    caps = np.stack(caps)
    od, fdd = _t(ctx, offs, torch.int32), _t(ctx, fds, torch.float64)
    hlay = Layout(0, n, n)
    hd, hptr = R.embed(ctx, None, hlay, "fc32", n=F)
    assert R.estimate_channel(ctx, ctx.to_device(caps), F, span, span, od, fdd, hptr) == 0
    ctx.synchronize()
    dense_hk = R.read_rows(hd, hlay, F)
    trn = orc.default_training(n)
    for f in range(F):
        assert rel_err(dense_hk[f], channel_estimate(orc, wide(caps[f]), offs[f], fds[f], trn, n)) <= TOL
    nd, nptr = R.embed(ctx, caps, Layout(0, span, span), "tone")
    assert R.normalize(ctx, nptr, F, span, span) == 0
    ctx.synchronize()
    dense_norm = R.read_rows(nd, Layout(0, span, span), F)
    for f in range(F):
        assert rel_err(dense_norm[f], orc.normalize(wide(caps[f]))) <= TOL
    buf = None
    try:
        buf = Far(ctx, caps, span, FAR_SAMPLES, "tone", torch.complex64)
        hf, hptr = R.embed(ctx, None, hlay, "fc32", n=F)
        assert R.estimate_channel(ctx, buf.ptr, F, FAR_SAMPLES, span, od, fdd, hptr) == 0
        ctx.synchronize()
        assert ctx.last_dispatch() == "k_sym<chest>"
        assert same(R.read_rows(hf, hlay, F), dense_hk) and R.only_rows_written(hf, hlay, F, "fc32")
        assert buf.windows_hold_the_fill() and buf.rows_hold(caps)
        assert R.normalize(ctx, buf.ptr, F, FAR_SAMPLES, span) == 0
        ctx.synchronize()
        assert ctx.last_dispatch() == ""
        assert same(buf.rows(), dense_norm) and buf.windows_hold_the_fill()
    finally:
        buf = None
        _release()
