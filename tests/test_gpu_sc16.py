"""EXT-9 on the GPU: sc16 (int16 I/Q) input.  Widening an int16 and multiplying once is exact IEEE arithmetic, so every sc16 entry point
must return BIT FOR BIT what its fc32 twin returns on the widened samples: no tolerance appears in this file.

References: the host functions (ofdm_sc16_widen / ofdm_sc16_narrow, held to tests/sc16_ref.py by tests/test_sc16_cpu.py) for the two
stages, and the project's own fc32 entry points on sc16_ref's widening (never the device's) of the same int16 samples for everything
else.  Every identity test draws its int16 input once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc16_ref  # noqa: E402
from tools.link import link as _link  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def bits(t):
    """the bit patterns of a float / complex tensor or array, on the host"""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8, 2: np.uint16}[a.dtype.itemsize if a.dtype.kind != "c" else a.dtype.itemsize // 2])


def rows_view(flat, base, n, ln, stride):
    """rows [n, ln(, 2)] of a flat device tensor of samples, row f starting at sample base + f * stride (a view, nothing copied)"""
    import torch

    if flat.dtype == torch.int16:
        return torch.as_strided(flat, (n, ln, 2), (2 * stride, 2, 1), 2 * base)
    return torch.as_strided(flat, (n, ln), (stride, 1), base)


# ------------------------------------------------------------------ 1. the stages
@pytest.mark.parametrize("frame_len", [1, 3, 4, 63, 64, 65, 1000])
def test_widen_and_narrow_stages_equal_the_host_functions(api, frame_len):
    """k_sc16_widen / k_sc16_narrow against ofdm_sc16_widen / ofdm_sc16_narrow, 5 rows, stride = length, length + 3 and length + 4,
    rows starting at an even and at an odd sample (16-byte accesses where base and strides allow, sample by sample for the rest and the ragged tail);
    nothing behind frame_len in an output row is written."""
    import torch

    ctx = api.Context(n_fft=64)
    rng = np.random.default_rng(900 + frame_len)
    n = 5
    for stride in (frame_len, frame_len + 3, frame_len + 4):    # + 4: rows apart, every row 16-byte aligned when the base is
        for base in (0, 1, 4):
            total = base + n * stride + 4
            q = rng.integers(-32768, 32768, (total, 2), dtype=np.int16)
            q[base] = (-32768, 32767)
            rows = np.stack([q[base + f * stride: base + f * stride + frame_len] for f in range(n)])
            for scale in (api.SC16_DEFAULT_SCALE, 3.1e-5):
                # widen
                out = torch.full((total,), complex(7.0, -7.0), dtype=torch.complex64, device=ctx.device)
                keep = out.clone()
                got = ctx.sc16_widen(rows_view(ctx.to_device(q), base, n, frame_len, stride), scale, out=rows_view(out, base, n, frame_len, stride))
                assert ctx.last_dispatch() == "k_sc16_widen"
                want = api.sc16_widen(rows, scale)
                assert np.array_equal(bits(got), bits(want)), ("widen", frame_len, stride, base, scale)
                mask = torch.ones(total, dtype=torch.bool, device=ctx.device)
                rows_view(mask, base, n, frame_len, stride)[:] = False
                assert np.array_equal(bits(out[mask]), bits(keep[mask])), ("widen wrote outside its rows", frame_len, stride, base)
            # narrow: values around +-full scale so that some components clip, with the edge inputs in row 0
            z = ((rng.standard_normal((total,)) + 1j * rng.standard_normal((total,))) * 0.5).astype(np.complex64)
            edge = np.array([0.5 / 30000, -1.5 / 30000, 32767.5 / 30000, np.inf, np.nan, -1e9], np.float32)
            z.view(np.float32)[2 * base: 2 * base + min(6, 2 * frame_len)] = edge[: min(6, 2 * frame_len)]
            zrows = np.stack([z[base + f * stride: base + f * stride + frame_len] for f in range(n)])
            out = torch.full((total, 2), 1234, dtype=torch.int16, device=ctx.device)
            keep = out.clone()
            got, clipped = ctx.sc16_narrow(rows_view(ctx.to_device(z), base, n, frame_len, stride), 30000.0, out=rows_view(out, base, n, frame_len, stride))
            assert ctx.last_dispatch() == "k_sc16_narrow"
            want = [api.sc16_narrow(zrows[f], 30000.0) for f in range(n)]
            assert np.array_equal(got.cpu().numpy(), np.stack([w[0] for w in want])), ("narrow", frame_len, stride, base)
            assert clipped.cpu().numpy().tolist() == [w[1] for w in want], ("clipped", frame_len, stride, base)
            mask = torch.ones(total, dtype=torch.bool, device=ctx.device)
            rows_view(mask, base, n, frame_len, stride)[:] = False
            assert torch.equal(out[mask], keep[mask]), ("narrow wrote outside its rows", frame_len, stride, base)
    if frame_len >= 63:
        assert sum(w[1] for w in want) > 0          # the count is exercised


def test_stage_argument_checks(api):
    import torch

    ctx = api.Context(n_fft=64)
    lib, h = ctx.lib, ctx.h
    q = torch.zeros((64, 2), dtype=torch.int16, device=ctx.device)
    z = torch.full((64,), complex(3.0, 3.0), dtype=torch.complex64, device=ctx.device)
    s = api.SC16_DEFAULT_SCALE
    # n_frames = 0: OK, nothing written (not even with NULL buffers)
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), 0, 8, 8, s, z.data_ptr(), 8) == 0
    assert lib.ofdm_sc16_widen_batch(h, None, 0, 8, 8, s, None, 8) == 0
    assert lib.ofdm_sc16_narrow_batch(h, z.data_ptr(), 0, 8, 8, 1.0, q.data_ptr(), 8, None) == 0
    ctx.synchronize()
    assert bool((z == complex(3.0, 3.0)).all()) and bool((q == 0).all())
    # stride < frame_len on either side, negative sizes, NULL buffers with work to do, a misaligned sc16 side
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), 2, 7, 8, s, z.data_ptr(), 8) == -1
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), 2, 8, 8, s, z.data_ptr(), 7) == -1
    assert lib.ofdm_sc16_narrow_batch(h, z.data_ptr(), 2, 7, 8, 1.0, q.data_ptr(), 8, None) == -1
    assert lib.ofdm_sc16_narrow_batch(h, z.data_ptr(), 2, 8, 8, 1.0, q.data_ptr(), 7, None) == -1
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), -1, 8, 8, s, z.data_ptr(), 8) == -1
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), 2, 8, -1, s, z.data_ptr(), 8) == -1
    assert lib.ofdm_sc16_widen_batch(h, None, 2, 8, 8, s, z.data_ptr(), 8) == -1
    assert lib.ofdm_sc16_narrow_batch(h, z.data_ptr(), 2, 8, 8, 1.0, None, 8, None) == -1
    assert lib.ofdm_sc16_widen_batch(h, q.data_ptr() + 2, 2, 8, 8, s, z.data_ptr(), 8) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ofdm_sc16_widen_batch(h, q.data_ptr(), 2, 8, 8, bad, z.data_ptr(), 8) == -1
        assert lib.ofdm_sc16_narrow_batch(h, z.data_ptr(), 2, 8, 8, bad, q.data_ptr(), 8, None) == -1
        assert lib.ofdm_rx_demod_sc16_batch(h, q.data_ptr(), 1, 64, 64, bad, 0, 0, None, None, None, 0, None, 64, None) == -1
    ctx.synchronize()
    assert bool((z == complex(3.0, 3.0)).all()) and bool((q == 0).all())


# ------------------------------------------------------------------ 2. the fused kernel, N = 64
def symbols_sc16(ctx, seed, n_sym, uniform=False):
    """(int16 [n_sym * S, 2], scale): n_sym symbols of the context's own TX path plus seeded noise, quantised at full scale (the largest
    component -> 32767; `scale` undoes it and is no power of two).  uniform: uniformly random int16 instead, both extremes included."""
    import torch

    rng = np.random.default_rng(seed)
    if uniform:
        q = rng.integers(-32768, 32768, (n_sym * ctx.S, 2), dtype=np.int16)
        q[0], q[1] = (-32768, 32767), (32767, -32768)
        return q, np.float32(1.0 / 32768.0)
    data = torch.from_numpy(rng.integers(0, 256, n_sym * ctx.bytes_per_symbol, dtype=np.uint8)).to(ctx.device)
    x = ctx.tx_symbols(data, n_sym).cpu().numpy().reshape(-1)
    sigma = 0.02 * float(np.sqrt(np.mean(np.abs(x) ** 2)))
    x = x + (sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))).astype(np.complex64)
    return sc16_ref.quantise(x, 1.0)


def channel_hk(seed, shape):
    rng = np.random.default_rng(seed)
    return (1.0 + 0.2 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)


def both_demods(ctx, q, scale, frames, row_syms, syms, sc16_rows=None, **kw):
    """rx_demod_sc16 on int16 rows and rx_demod on sc16_ref's widening of the same rows -> (got, want, dispatch of the sc16 call)"""
    S = ctx.S
    qd = ctx.to_device(q[: frames * row_syms * S].reshape(frames, row_syms * S, 2)) if sc16_rows is None else sc16_rows
    wide = ctx.to_device(sc16_ref.widen(q[: frames * row_syms * S], scale).reshape(frames, row_syms * S))
    want = ctx.rx_demod(wide, syms, **kw)
    got = ctx.rx_demod_sc16(qd, syms, scale=float(scale), **kw)
    return got, want, ctx.last_dispatch()


def same(got, want):
    if isinstance(got, tuple):
        return all(same(g, w) for g, w in zip(got, want))
    return np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("guard", [False, True], ids=["full", "guard"])
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_fused_demod_is_the_fc32_kernel_on_the_widened_samples(api, mod, guard):
    """5 frames of 8 symbols = 5 groups: more than a workgroup's four wavefronts and no multiple of four.  H absent (scale: the
    quantiser's, and the default), H shared (also with a scale that is no power of two), first_symbol = 3."""
    ctx = api.Context(n_fft=64, modulation=mod, guard_bands=guard)
    q, scale = symbols_sc16(ctx, 1600 + 10 * mod + guard, 5 * 11)
    hk = ctx.to_device(channel_hk(7, 64))
    for kw, sc in (({}, scale), ({}, api.SC16_DEFAULT_SCALE), ({"hk": hk}, api.SC16_DEFAULT_SCALE), ({"hk": hk}, 3.1e-5)):
        got, want, disp = both_demods(ctx, q, sc, 5, 8, 8, **kw)
        assert disp == "k_demod64_sc16", disp
        assert same(got, want), (mod, guard, list(kw), sc)
    got, want, disp = both_demods(ctx, q, scale, 5, 11, 8, first_symbol=3)
    assert disp == "k_demod64_sc16" and same(got, want)


def test_fused_demod_rows_at_odd_samples_and_full_range_input(api):
    """The new alignment freedom: rows an odd number of samples apart that start at an odd sample (4-byte aligned only), on TX symbols
    and on uniformly random int16 with both extremes."""
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    for uniform in (False, True):
        q, scale = symbols_sc16(ctx, 1700, 40, uniform=uniform)
        stride, base = 8 * 80 + 1, 3
        flat = np.zeros((base + 5 * stride, 2), np.int16)
        for f in range(5):
            flat[base + f * stride: base + f * stride + 640] = q[f * 640:(f + 1) * 640]
        rows = rows_view(ctx.to_device(flat), base, 5, 640, stride)
        assert rows.data_ptr() % 8 == 4
        got, want, disp = both_demods(ctx, q, scale, 5, 8, 8, sc16_rows=rows)
        assert disp == "k_demod64_sc16" and same(got, want), uniform


@pytest.mark.parametrize("groups,want_kernel", [(4, "k_demod64_sc16<burst4>"), (8, "k_demod64_sc16<burst8>"), (16, "k_demod64_sc16<burst16>"),
                                                (128, "k_demod64_sc16<burst16>")])
def test_fused_demod_bursts(api, groups, want_kernel):
    """The config-2 shape (64-QAM, guard bands, contiguous 128-byte aligned output) just large enough for each burst length; 128 groups
    of 2 a frame on one workgroup: a burst spans 8 frames and every wavefront takes two."""
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning={"grid_cap": 1} if groups == 128 else None)
    syms = 16 if groups == 128 else 8
    frames = groups * 8 // syms
    q, scale = symbols_sc16(ctx, 1800 + groups, frames * syms)
    got, want, disp = both_demods(ctx, q, scale, frames, syms, syms)
    assert got.data_ptr() % 128 == 0 and disp == want_kernel, disp
    assert ctx.last_dispatch() == want_kernel and same(got, want)
    ctx.set_tuning("demod64_burst", 1)
    got1, _, disp = both_demods(ctx, q, scale, frames, syms, syms)
    assert disp == "k_demod64_sc16" and same(got1, want)


# ------------------------------------------------------------------ 3. everything else: k_sc16_widen + the fc32 path
def test_fallbacks_widen_and_take_the_fc32_path(api):
    import torch

    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    q, scale = symbols_sc16(ctx, 1900, 5 * 10)
    off = torch.tensor([0, 3, 17, 40, 80], dtype=torch.int32, device=ctx.device)
    fd = torch.tensor([0.0, 1e-3, -2e-3, 3e-4, -1e-4], dtype=torch.float64, device=ctx.device)
    hk5 = ctx.to_device(channel_hk(8, (5, 64)))
    cases = {
        "nine symbols": dict(row_syms=9, syms=9),
        "offset and f_delta": dict(row_syms=10, syms=8, offset=off, f_delta=fd),
        "per-frame hk": dict(row_syms=8, syms=8, hk=hk5),
        "soft": dict(row_syms=8, syms=8, want_soft=True),
        "cut tail": dict(row_syms=8, syms=8, frame_len=8 * 80 - 20),
        "everything, chunked": dict(row_syms=10, syms=9, offset=off, f_delta=fd, hk=hk5, want_soft=True),
    }
    for chunk in (0, 1, 2):
        ctx.set_tuning("sc16_chunk_frames", chunk)
        for what, kw in cases.items():
            kw = dict(kw)
            row_syms, syms = kw.pop("row_syms"), kw.pop("syms")
            got, want, disp = both_demods(ctx, q, scale, 5, row_syms, syms, **kw)
            assert disp.split("+")[0] == "k_sc16_widen" and len(disp.split("+")) >= 2 and disp.count("k_sc16_widen") == 1, (what, disp)
            assert same(got, want), (what, chunk)
    ctx.set_tuning("sc16_chunk_frames", 0)
    ctx.set_tuning("no_demod64_sc16", 1)                       # the A/B key: the widen path inside the fused kernel's envelope
    got, want, disp = both_demods(ctx, q, scale, 5, 8, 8)
    assert disp == "k_sc16_widen+k_demod64" and same(got, want)
    ctx.set_tuning("no_demod64_sc16", 0)
    got, want, disp = both_demods(ctx, q, scale, 5, 8, 8)
    assert disp == "k_demod64_sc16" and same(got, want)


@pytest.mark.parametrize("n_fft", [128, 1024, 4096])
def test_other_transform_lengths_go_through_the_widen_path(api, n_fft):
    ctx = api.Context(n_fft=n_fft, modulation=api.QAM16, guard_bands=True)
    q, scale = symbols_sc16(ctx, 2000 + n_fft, 2 * 4)
    got, want, disp = both_demods(ctx, q, scale, 2, 4, 4)
    assert disp.split("+")[0] == "k_sc16_widen" and same(got, want), disp
    ctx.rx_demod(ctx.to_device(sc16_ref.widen(q, scale).reshape(2, -1)), 4)
    assert disp == "k_sc16_widen+" + ctx.last_dispatch(), (disp, ctx.last_dispatch())   # the same kernel as the fc32 call on those rows


# ------------------------------------------------------------------ 4. the decode chain
def decode_case(api, ecc, n, mod, **ctx_kw):
    """16 frames of tools/link.py's seeded link, one empty slot, one frame cut by the end of its capture, quantised with the capture's
    peak at 0.9 of full scale -> (context, int16 captures on the device, scale, widened captures on the device, symbols)"""
    c, pay, rx, D = _link(ecc, n, mod, 16, 100, 25.0, 160 + n + ecc, guard=True, tuning={"sc16_chunk_frames": 5}, **ctx_kw)
    rx = rx.clone()
    rx[3].zero_()
    shift = rx.shape[1] - 4 * c.S
    rx[9, shift:] = rx[9, : rx.shape[1] - shift].clone()
    rx[9, :shift].zero_()
    q, scale = sc16_ref.quantise(rx.cpu().numpy(), 0.9)
    assert 0.89 * 32767 <= np.abs(q.astype(np.int32)).max() <= 0.9 * 32767 + 1
    return c, c.to_device(q), float(scale), c.to_device(sc16_ref.widen(q, scale)), D


@pytest.mark.parametrize("ecc,n,mod,ctx_kw", [
    (0, 64, 4, {}),                       # ECC_NONE
    (80, 64, 4, {}),                      # LDPC648 with the frame check
    (12, 64, 4, {"chest_mode": 1}),       # CONV_K7F_R34, denoised channel estimate
    (0, 256, 2, {"cfo_mode": 3}),         # ECC_NONE at N = 256, wide CFO acquisition
], ids=["none64", "ldpc648fcs", "k7f_r34_wls", "none256_cfowide"])
def test_decode_chain_equals_decode_batch_on_the_widened_capture(api, ecc, n, mod, ctx_kw):
    c, qd, scale, wide, D = decode_case(api, ecc, n, mod, **ctx_kw)
    want = c.decode_batch(wide, max_symbols=D)
    got = c.decode_batch_sc16(qd, max_symbols=D, scale=scale)
    disp = c.last_dispatch()
    assert disp.split("+")[0] == "k_sc16_widen" and len(disp.split("+")) > 2, disp
    for k in ("status", "len", "offset"):
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k
    assert np.array_equal(bits(got["f_delta"]), bits(want["f_delta"])) and np.array_equal(bits(got["metric"]), bits(want["metric"]))
    ln = want["len"].cpu().numpy()
    gb, wb = got["bytes"].cpu().numpy(), want["bytes"].cpu().numpy()
    for f in range(16):
        assert bytes(gb[f, : ln[f]]) == bytes(wb[f, : ln[f]]), f
    st = want["status"].cpu().numpy()
    assert st[3] != 0 and st[9] != 0 and (st == 0).sum() >= 12, st


# ------------------------------------------------------------------ 5. the host path
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_calls_equal_the_device_calls(api, pinned):
    c, qd, scale, _, D = decode_case(api, 0, 64, 6)
    q7 = qd[:7].cpu().numpy()
    caps = api.pinned_empty(q7.shape, np.int16) if pinned else np.zeros(q7.shape, np.int16)
    caps[:] = q7
    want = {k: v.cpu().numpy() for k, v in c.decode_batch_sc16(qd[:7].contiguous(), max_symbols=D, scale=scale).items()}
    nsym = q7.shape[1] // 80 // 8 * 8                         # regular streams of whole 8-symbol groups: the fused kernel per chunk
    sym = api.pinned_empty((7, nsym * 80, 2), np.int16) if pinned else np.zeros((7, nsym * 80, 2), np.int16)
    sym[:] = q7[:, : nsym * 80]
    want_b = c.rx_demod_sc16(c.to_device(np.ascontiguousarray(sym)), nsym, scale=scale).cpu().numpy()
    assert c.last_dispatch().startswith("k_demod64_sc16")
    for chunk in (1, 3, 0):
        got = c.decode_host_sc16(caps, max_symbols=D, chunk_frames=chunk, scale=scale)
        for k in ("status", "len", "offset"):
            assert np.array_equal(got[k], want[k]), (chunk, k)
        assert np.array_equal(bits(got["f_delta"]), bits(want["f_delta"])) and np.array_equal(bits(got["metric"]), bits(want["metric"]))
        for f in range(7):
            assert bytes(got["bytes"][f, : got["len"][f]]) == bytes(want["bytes"][f, : want["len"][f]]), (chunk, f)
        assert np.array_equal(c.demod_host_sc16(sym, nsym, chunk_frames=chunk, scale=scale), want_b), ("demod", chunk)


def test_host_calls_reject_bad_arguments(api):
    ctx = api.Context(n_fft=64, modulation=api.QPSK)
    x = np.zeros((2, 1000, 2), np.int16)
    out = np.zeros((2, 8), np.uint8)
    ln = np.zeros(2, np.int32)
    st = np.zeros(2, np.int32)
    lib, h, s = ctx.lib, ctx.h, api.SC16_DEFAULT_SCALE
    dec = lambda *a: lib.ofdm_rx_decode_sc16_host(h, *a, out.ctypes.data, 8, ln.ctypes.data, st.ctypes.data, None, None, None, 0)
    assert dec(x.ctypes.data, 2, 500, 1000, s, 0, 4) == -1      # rows of a host batch must not overlap
    assert dec(x.ctypes.data, 2, 1000, 1000, s, 0, 40) == -1    # the output row must hold max_symbols of payload
    assert dec(None, 2, 1000, 1000, s, 0, 1) == -1              # NULL mandatory pointer
    assert dec(x.ctypes.data, 2, 1000, 1000, 0.0, 0, 1) == -1   # scale
    assert dec(x.ctypes.data, 0, 1000, 1000, s, 0, 1) == 0
    dem = lambda *a: lib.ofdm_rx_demod_sc16_host(h, *a)
    assert dem(x.ctypes.data, 2, 500, 1000, s, 0, 1, out.ctypes.data, 16, 0) == -1
    assert dem(x.ctypes.data, 2, 1000, 1000, s, 0, 1, out.ctypes.data, 8, 0) == -1    # out_stride < bytes of a row
    assert dem(None, 2, 1000, 1000, s, 0, 1, out.ctypes.data, 16, 0) == -1
    assert dem(x.ctypes.data, 2, 1000, 1000, float("nan"), 0, 1, out.ctypes.data, 16, 0) == -1
    assert dem(x.ctypes.data, 0, 1000, 1000, s, 0, 1, out.ctypes.data, 16, 0) == 0


# ------------------------------------------------------------------ 6. end to end
def test_encode_narrow_decode_returns_the_payload(api):
    """api.encode -> sc16_narrow at the frame's own peak -> api.decode of the int16 array: 64-QAM, LDPC648 with the frame check, no
    channel."""
    pay = bytes(np.random.default_rng(21).integers(0, 256, 300, dtype=np.uint8))
    tx = api.encode(pay, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True)
    peak = float(max(np.abs(tx.real).max(), np.abs(tx.imag).max()))
    q, clipped = api.sc16_narrow(tx, 32767.0 / peak)
    assert q.shape == (tx.size, 2) and q.dtype == np.int16 and clipped == 0 and np.abs(q.astype(np.int32)).max() == 32767
    assert api.decode(q, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True) == pay
    assert api.decode(q, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True, scale=peak / 32767.0) == pay
