"""k_sym<llr> against the f64 oracle.  Every expected value here comes from oracle/ofdm_oracle.c and numpy (tests/soft_ref.py): the
equalised points of orc.rx_demod / orc.decode_given, the channel of orc.estimate_channel, the brute-force max-log LLR.  The rule is
soft_ref.llr_compare: an LLR equals quantise(y) unless the f64 product y lies within eps of a rounding boundary, eps being the
project's 1e-5 point tolerance carried through the derivative of y (soft_ref's docstring); at most CAP of a case's elements may be
that close.  Every call runs on the device-sized grid and on grids of 1 and 3 workgroups (tuning key grid_cap), which make every
workgroup of the persistent kernel take several steps; the three results must be the same bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_ref as sr  # noqa: E402
from util import fc32, make_symbols_np, through_channel, wide  # noqa: E402

pytestmark = pytest.mark.gpu

MODS = (1, 2, 4, 6, 8)
SNRS = (30.0, 14.0, 6.0)
CAPS = (0, 1, 3)
CAP = 0.02          # largest share of a case's elements that may lie within eps of a rounding boundary (a condition of the inputs)
SCALE = 32.0
# (frames, symbols per frame) per N: with G = 256 / (N / 8) symbols per workgroup step (32, 16, 8, 4, 2, 1, 1) the batch is nine or
# more steps' worth -- three steps for each of three workgroups -- and its last step is partial wherever G > 1
SHAPES = {64: (5, 53), 128: (5, 27), 256: (5, 13), 512: (5, 7), 1024: (7, 3), 2048: (3, 3), 4096: (3, 3)}


def _api():
    from ofdm_amd import api

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return api


def _steps(n, total):
    g = max(1, 256 // (n // 8))
    return g, (total + g - 1) // g


def _channels(orc, rng, n, n_frames):
    per_frame = fc32(1.0 + 0.3 * (rng.standard_normal((n_frames, n)) + 1j * rng.standard_normal((n_frames, n))))
    return {"none": None, "shared": fc32(np.fft.fft(orc.channel_taps(), n)), "per frame": per_frame}


def stream_case(orc, rng, n, guard, mod, snr, hk, scale=SCALE, shape=None):
    """-> (fc32 samples [F, D * S] for the GPU, the oracle's side of the same call); no GPU involved"""
    F, D = shape or SHAPES[n]
    x, _ = make_symbols_np(orc, rng, F * D, n, guard, mod, snr_db=snr)
    x = x.reshape(F, -1)
    if hk is not None:
        x = sr.through_h(x, n, hk.reshape(-1, n))
    return x, sr.oracle_llr_reference(orc, x, n, guard, mod, scale, hk)


def _run_caps(ctx, call):
    """call() on the device-sized grid, on 1 and on 3 workgroups -> the first result, after requiring all three to be the same bytes"""
    outs = []
    for cap in CAPS:
        ctx.set_tuning("grid_cap", cap)
        outs.append(call())
        assert ctx.last_dispatch() == "k_sym<llr>", ctx.last_dispatch()
    ctx.set_tuning("grid_cap", 0)
    ctx.synchronize()
    for cap, o in zip(CAPS[1:], outs[1:]):
        assert torch.equal(o, outs[0]), f"grid_cap {cap} changes the LLRs"
    return outs[0].cpu().numpy()


def _hold(got, ref, what):
    share = sr.llr_compare(got, ref["y"], ref["eps"], what=what)
    sr.assert_signs(got, ref, what)
    n_exact = int(sr.llr_decided(ref["y"], ref["eps"]).sum())
    print(f"{what}: excused {100 * share:.3f} %, {n_exact} of {got.size} compared exactly, {int((np.abs(got) == 127).sum())} saturated")
    assert share <= CAP, (what, share)
    return share


# ---------------------------------------------------------------------------------------------------------- a. symbol streams
@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_stream_llrs_equal_the_oracle(orc, n, guard):
    api = _api()
    rng = np.random.default_rng(4000 + n + guard)
    F, D = SHAPES[n]
    g, groups = _steps(n, F * D)
    assert groups >= 9 and (g == 1 or (F * D) % g != 0), (n, g, groups)
    worst = (0.0, None)
    for mod in MODS:
        ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
        for name, hk in _channels(orc, rng, n, F).items():
            hd = None if hk is None else ctx.to_device(hk)
            for snr in SNRS:
                x, ref = stream_case(orc, rng, n, guard, mod, snr, hk)
                xd = ctx.to_device(x)
                got = _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=hd))
                what = f"stream N {n} guard {guard} mod {mod} {snr} dB H {name}"
                worst = max(worst, (_hold(got, ref, what), what))
    print("largest excused share:", worst)


# ---------------------------------------------------------------------------------------------------------- b. row layout
@pytest.mark.parametrize("n,mod,guard", [(64, 6, True), (512, 1, False), (1024, 4, True), (4096, 2, False)])
def test_row_stride_and_alignment_do_not_change_the_llrs(orc, n, mod, guard):
    api = _api()
    rng = np.random.default_rng(4100 + n)
    F, D = SHAPES[n]
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 3})
    hk = _channels(orc, rng, n, F)["per frame"]
    x, ref = stream_case(orc, rng, n, guard, mod, 14.0, hk)
    xd, hd = ctx.to_device(x), ctx.to_device(hk)
    tight = ctx.rx_llr(xd, D, hk=hd)
    assert tight.data_ptr() % 16 == 0 and tight.stride(0) % 16 == 0
    _hold(tight.cpu().numpy(), ref, f"rows N {n} tight")
    nl = tight.shape[1]
    SENT = -128                                                    # never a legal LLR
    # (base offset, row stride): 16-byte stores with slack; odd stride; odd base; both odd
    for off, stride in ((0, nl + 32), (16, nl + 48), (0, nl + 5), (7, nl + 16), (3, nl + 1), (1, nl)):
        buf = torch.full((off + F * stride + 64,), SENT, dtype=torch.int8, device=ctx.device)
        rows = buf[off:off + F * stride].view(F, stride)
        out = ctx.rx_llr(xd, D, hk=hd, out=rows[:, :nl])
        assert ctx.last_dispatch() == "k_sym<llr>"
        assert out.data_ptr() == buf.data_ptr() + off and ((out.data_ptr() | stride) % 16 == 0) == ((off, stride) in ((0, nl + 32), (16, nl + 48)))
        assert torch.equal(rows[:, :nl], tight), (off, stride)
        assert bool((rows[:, nl:] == SENT).all()) and bool((buf[:off] == SENT).all()) and bool((buf[off + F * stride:] == SENT).all()), (off, stride)
    with pytest.raises(api.OfdmError):
        ctx.rx_llr(xd, D, hk=hd, out=torch.empty((F, nl - 1), dtype=torch.int8, device=ctx.device))


# ---------------------------------------------------------------------------------------------------------- c. frame mode
def frame_case(orc, rng, n, mod, guard, nbytes, F=5):
    """Captures as the decode chain sees them, and the oracle's side of rx_llr on them; no GPU involved.  Timing and CFO are the
    oracle's own (decode_sc), the channel is orc.estimate_channel on the oracle's derotated training blocks, the points are
    decode_given's.  -> (captures fc32 [F, span], frame_len, D, offsets, f_deltas, f64 channels [F, n], reference)"""
    S = n + n // 4
    flen = orc.frame_len(nbytes, n, guard, mod)
    D = flen // S - 10
    g, groups = _steps(n, F * D)
    assert groups >= 7 and (g == 1 or (F * D) % g != 0), (n, g, F * D)   # three workgroups take two or three steps each, the last one partial
    span = flen + 2 * S
    delays = [3, S // 4, 17, S // 2 + S // 4, S - 5]
    frame_len = flen + S // 2                                      # the late frames lose a good part of their last symbol
    caps = np.stack([through_channel(orc, rng, orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, n), span, d,
                                     (rng.random() * 1.6 - 0.8) * np.pi / S, 22.0, data_start=10 * S) for d in delays[:F]])
    bins = sr.data_bins(orc, n, guard)
    offs, fds, hks, pts = [], [], [], []
    for f in range(F):
        c = wide(caps[f])
        c[frame_len:] = 0                                          # what the kernel reads past frame_len
        w = orc.decode_sc(c, guard, mod, n, max_symbols=D)
        assert w["status"] == 0, (f, w["status"])
        g = orc.decode_given(c, w["offset"], w["f_delta"], guard, mod, n, max_symbols=D, want_soft=True)
        assert g["n_symbols"] == D
        rot = orc.cfo_rotate(c[w["offset"]:w["offset"] + 10 * S], w["f_delta"], 0)
        hks.append(orc.estimate_channel(rot[5 * S:], orc.default_training(n), n))
        offs.append(w["offset"]); fds.append(w["f_delta"]); pts.append(np.asarray(g["soft"]).reshape(D, len(bins)))
    assert max(offs) + (10 + D) * S > frame_len + S // 8 and min(offs) + (10 + D) * S <= frame_len, offs   # a cut frame and a whole one
    hks, pts = np.stack(hks), np.stack(pts)
    wts = sr.channel_weights(hks, bins)
    ref = {"y": sr.frame_llrs_unrounded(pts, mod, SCALE, wts), "eps": sr.llr_eps(pts, mod, SCALE, wts, np.abs(hks[:, bins])),
           "bits": np.stack([sr.unpack_bits(np.frombuffer(orc.demodulate(p.ravel(), mod), np.uint8)) for p in pts])}
    return caps, frame_len, D, offs, fds, hks, ref


FRAME_CASES = [(64, 6, True, 1500), (256, 8, False, 2500), (1024, 4, True, 1100), (4096, 2, False, 2500)]


@pytest.mark.parametrize("n,mod,guard,nbytes", FRAME_CASES)
def test_frame_mode_llrs_equal_the_oracle_chain(orc, n, mod, guard, nbytes):
    """rx_llr as the decode chain calls it: first_symbol = 10, per-frame offset and CFO, a per-frame estimated channel (the fc32
    rounding of the oracle's), frame_len inside the last symbol of the late frames, against frame_case's reference."""
    api = _api()
    rng = np.random.default_rng(4200 + n)
    caps, frame_len, D, offs, fds, hks, ref = frame_case(orc, rng, n, mod, guard, nbytes)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    assert (D, caps.shape[1]) == (ctx.data_symbols(nbytes), ctx.frame_samples(nbytes) + 2 * ctx.S)
    xd, hd = ctx.to_device(caps), ctx.to_device(fc32(hks))
    od, fd = torch.tensor(offs, dtype=torch.int32, device=ctx.device), torch.tensor(fds, dtype=torch.float64, device=ctx.device)
    got = _run_caps(ctx, lambda: ctx.rx_llr(xd, D, first_symbol=10, offset=od, f_delta=fd, hk=hd, frame_len=frame_len))
    _hold(got, ref, f"frame mode N {n} mod {mod} guard {guard}")


# ---------------------------------------------------------------------------------------------------------- d. llr_scale
@pytest.mark.parametrize("scale", [2.0 ** -3, 32.0, 2.0 ** 12])
@pytest.mark.parametrize("mod,n,guard", [(1, 128, True), (2, 512, False), (4, 2048, True), (6, 64, True), (8, 1024, False)])
def test_llr_scales(orc, mod, n, guard, scale):
    api = _api()
    rng = np.random.default_rng(4300 + n)
    F, D = SHAPES[n]
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    hk = _channels(orc, rng, n, F)["per frame"]
    x, ref = stream_case(orc, rng, n, guard, mod, 14.0, hk, scale=scale)
    xd, hd = ctx.to_device(x), ctx.to_device(hk)
    got = _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=hd, scale=scale))
    _hold(got, ref, f"scale {scale} N {n} mod {mod}")
    sat = float((np.abs(sr.quantise(ref["y"])) == 127).mean())     # of the reference: all small, mixed, almost all saturated
    assert (sat == 0.0) if scale < 1 else (sat > 0.9) if scale > 1000 else (0.0 < sat < 0.9 or mod < 4), (scale, sat)


# ---------------------------------------------------------------------------------------------------------- e. degenerate inputs
@pytest.mark.parametrize("n,mod,guard", [(64, 6, True), (1024, 4, False), (256, 1, True)])
def test_dead_carriers_and_dead_channels(orc, n, mod, guard):
    api = _api()
    rng = np.random.default_rng(4400 + n)
    F, D = SHAPES[n]
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    bins = sr.data_bins(orc, n, guard)
    hk = _channels(orc, rng, n, F)["per frame"]
    x, _ = stream_case(orc, rng, n, guard, mod, 14.0, hk)          # the symbols went through the live channel ...
    dead = [bins[0], bins[5], bins[-1]]
    hk = hk.copy()
    hk[:, dead] = 0                                                # ... and the receiver is told that three data carriers are dead
    hk[1, bins[7]] = 0                                             # one more in frame 1 only
    ref = sr.oracle_llr_reference(orc, x, n, guard, mod, SCALE, hk)
    assert not np.isfinite(ref["y"]).all()
    xd, hd = ctx.to_device(x), ctx.to_device(hk)
    got = _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=hd))
    g4 = got.reshape(F, D, len(bins), mod)
    assert (g4[:, :, [0, 5, len(bins) - 1], :] == 0).all() and (g4[1, :, 7, :] == 0).all() and (g4[0, :, 7, :] != 0).any()
    _hold(got, ref, f"dead carriers N {n} mod {mod}")              # the live carriers, with w over all data carriers
    x4 = ctx.to_device(fc32(4.0 * wide(x)))
    h4 = ctx.to_device(fc32(4.0 * wide(hk)))
    assert np.array_equal(_run_caps(ctx, lambda: ctx.rx_llr(x4, D, hk=h4)), got)   # gain 4 on both: same points, same w, same L
    zero = torch.zeros((F, n), dtype=torch.complex64, device=ctx.device)
    assert not _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=zero)).any()
    assert not _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=zero[0].contiguous())).any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("n,mod,guard,with_h", [(64, 6, True, True), (512, 2, False, False), (2048, 8, True, True), (128, 1, True, False)])
def test_a_non_finite_sample_zeroes_its_symbol_only(orc, n, mod, guard, with_h, bad):
    api = _api()
    rng = np.random.default_rng(4500 + n)
    F, D = SHAPES[n]
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    hk = _channels(orc, rng, n, F)["per frame"] if with_h else None
    x, _ = stream_case(orc, rng, n, guard, mod, 14.0, hk)
    xd = ctx.to_device(x)
    hd = None if hk is None else ctx.to_device(hk)
    clean = _run_caps(ctx, lambda: ctx.rx_llr(xd, D, hk=hd))
    f, k = 2, D // 2
    xb = xd.clone()
    xb[f, k * S + S // 4 + 5] = complex(bad, bad)                  # inside the symbol's FFT window (past its cyclic prefix)
    got = _run_caps(ctx, lambda: ctx.rx_llr(xb, D, hk=hd))
    nl = got.shape[1] // D
    assert not got[f, k * nl:(k + 1) * nl].any()
    want = clean.copy()
    want[f, k * nl:(k + 1) * nl] = 0
    assert np.array_equal(got, want) and clean[f, k * nl:(k + 1) * nl].any()
