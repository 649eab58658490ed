"""GPU parity: every HIP stage and both pipelines, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Bars (BASELINE.json north_star): bit-exact QAM hard-decision indices / decoded bytes / timing
indices; <= 1e-5 norm-relative on complex FFT / correlation / channel samples (f32 kernels vs f64 oracle).
"""
import numpy as np
import pytest

from util import (SC80_SEARCHES, assert_bytes_match, fc32, long_period_captures, loud_payload, make_capture, make_symbols,
                  make_symbols_np, rel_err, sc80_corner_captures, through_channel, wide)

pytestmark = pytest.mark.gpu
TOL = 1e-5  # north_star tolerance for complex samples


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def dev(ctx, a):
    return ctx.to_device(a)


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ a8: fft / ifft
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_fft_ifft(api, orc, n):
    rng = np.random.default_rng(n)
    ctx = api.Context(n_fft=n)
    nvec = 37 if n <= 512 else 5
    x = fc32(rng.standard_normal((nvec, n)) + 1j * rng.standard_normal((nvec, n)))
    X = host(ctx.fft(dev(ctx, x)))
    Xi = host(ctx.fft(dev(ctx, x), inverse=True))
    ctx.synchronize()
    for v in range(nvec):
        assert rel_err(X[v], orc.fft(wide(x[v]))) <= TOL
        assert rel_err(Xi[v], orc.fft(wide(x[v]), inverse=True)) <= TOL
    # in place
    t = dev(ctx, x)
    ctx.fft(t, out=t)
    assert np.array_equal(host(t), X)


# ------------------------------------------------------------------ a7 / a17: prefix_block / unprefix_block
@pytest.mark.parametrize("n", [64, 1024])
def test_prefix_unprefix(api, orc, n):
    rng = np.random.default_rng(n + 1)
    ctx = api.Context(n_fft=n)
    f = fc32(rng.standard_normal((9, n)) + 1j * rng.standard_normal((9, n)))
    blocks = host(ctx.prefix_block(dev(ctx, f)))
    assert blocks.shape == (9, n + n // 4)
    for v in range(9):
        assert rel_err(blocks[v], orc.prefix_block(wide(f[v]))) <= TOL
        np.testing.assert_array_equal(blocks[v][: n // 4], blocks[v][n:])  # cyclic prefix is a copy
    back = host(ctx.unprefix_block(dev(ctx, blocks)))
    for v in range(9):
        assert rel_err(back[v], orc.unprefix_block(wide(blocks[v]), n)) <= TOL
        assert rel_err(back[v], f[v]) <= 4 * TOL  # round trip


# ------------------------------------------------------------------ a5 / a20 + EXT-1: modulate / demodulate
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_modulate_demodulate(api, orc, mod):
    rng = np.random.default_rng(mod)
    ctx = api.Context(modulation=mod)
    data = rng.integers(0, 256, 600, dtype=np.uint8)
    pts = host(ctx.modulate(dev(ctx, data)))
    want = orc.modulate(bytes(data), mod)
    assert pts.shape == want.shape
    np.testing.assert_array_equal(pts, want.astype(np.complex64))  # levels are exactly representable up to f32 rounding
    noisy = fc32(want + (rng.standard_normal(want.size) + 1j * rng.standard_normal(want.size)) * 0.3 / (1 << (mod // 2 or 1)))
    by, idx = ctx.demodulate(dev(ctx, noisy), want_indices=True)
    assert bytes(host(by)) == orc.demodulate(wide(noisy), mod)
    np.testing.assert_array_equal(host(idx), orc.demap_indices(wide(noisy), mod))
    assert bytes(host(ctx.demodulate(dev(ctx, pts)))) == bytes(data)
    with pytest.raises(api.OfdmError):
        ctx.demodulate(dev(ctx, pts[:7]))  # receiver.rs:153 assert


def test_qpsk_reference_kats(api, orc):
    ctx = api.Context(modulation=api.QPSK)
    # src/lib.rs:37-51 and the 0x61 KAT of transmitter.rs:122-133
    t = dev(ctx, np.frombuffer(b"alskdjas", np.uint8).copy())
    assert bytes(host(ctx.demodulate(ctx.modulate(t)))) == b"alskdjas"
    assert list(host(ctx.modulate(dev(ctx, np.array([0x61], np.uint8))))) == [1 - 1j, -1 - 1j, -1 + 1j, 1 - 1j]
    # tie rules Q6 (receiver.rs:169-175)
    pts = np.array([0 + 0j, 1 + 0j, -1 + 0j, 0 - 1j, -1 + 1j, -1 - 1j, complex(-0.0, 0.0), complex(1, np.nan)], np.complex64)
    _, idx = ctx.demodulate(dev(ctx, pts), want_indices=True)
    assert list(host(idx)) == [3, 3, 0, 1, 2, 0, 3, 0] == list(orc.demap_indices(wide(pts), orc.QPSK))


# ------------------------------------------------------------------ a6 / a9
def test_encode_block_and_normalize(api, orc):
    rng = np.random.default_rng(2)
    for n, guard in ((64, True), (64, False), (256, True)):
        ctx = api.Context(n_fft=n, guard_bands=guard)
        nd = ctx.data_carriers
        d = fc32(rng.standard_normal((5, nd)) + 1j * rng.standard_normal((5, nd)))
        bins = host(ctx.encode_block(dev(ctx, d)))
        for s in range(5):
            want, used = orc.encode_block(wide(d[s]), n, guard)
            assert used == nd
            np.testing.assert_array_equal(bins[s], want.astype(np.complex64))
    ctx = api.Context()
    x = fc32(rng.standard_normal((3, 1000)) + 1j * rng.standard_normal((3, 1000)))
    y = host(ctx.normalize(dev(ctx, x)))
    for r in range(3):
        assert rel_err(y[r], orc.normalize(wide(x[r]))) <= TOL
        assert max(y[r].real.max(), y[r].imag.max()) == 1.0


# ------------------------------------------------------------------ EXT-2: Hamming(7,4)
def test_hamming74(api, orc):
    rng = np.random.default_rng(3)
    ctx = api.Context()
    for n in (4, 64, 1001):
        data = rng.integers(0, 256, n, dtype=np.uint8)
        code = host(ctx.hamming74_encode(dev(ctx, data)))
        assert bytes(code) == orc.hamming74_encode(bytes(data))
        bits = np.unpackbits(code, bitorder="little").copy()
        for cw in range(bits.size // 7):
            if cw % 3:
                bits[cw * 7 + int(rng.integers(0, 7))] ^= 1
        bad = np.packbits(bits, bitorder="little")
        dec, fixed = ctx.hamming74_decode(dev(ctx, bad))
        want, want_fixed = orc.hamming74_decode(bytes(bad))
        assert bytes(host(dec)) == want and int(host(fixed)[0]) == want_fixed
        assert want[:n] == bytes(data)


@pytest.mark.parametrize("grid_cap", [0, 1])
def test_hamming74_decode_every_seven_bit_word(api, orc, grid_cap):
    """All 128 seven-bit words -- the 16 code words, their 112 single-error neighbours, which are every other word: a double error
    decodes to a wrong nibble, and only the oracle says which -- in each of the eight code-word slots of a 7-byte block, the other
    seven slots holding valid code words: 1 024 blocks through k_ham_decode, bytes and `fixed` count against the oracle."""
    rng = np.random.default_rng(74)
    ctx = api.Context(tuning={"grid_cap": grid_cap} if grid_cap else None)
    data = rng.integers(0, 256, 4 * 8 * 128, dtype=np.uint8)
    words = np.unpackbits(np.frombuffer(orc.hamming74_encode(bytes(data)), np.uint8), bitorder="little").reshape(8 * 128, 8, 7).copy()
    for slot in range(8):
        for w in range(128):
            words[slot * 128 + w, slot] = [(w >> b) & 1 for b in range(7)]
    code = np.packbits(words.reshape(-1), bitorder="little")
    assert code.size == 7 * 1024
    dec, fixed = ctx.hamming74_decode(dev(ctx, code))
    want, want_fixed = orc.hamming74_decode(bytes(code))
    got = host(dec)
    assert got.size == len(want) == 4 * 1024
    bad = np.nonzero(got.reshape(1024, 4) != np.frombuffer(want, np.uint8).reshape(1024, 4))[0]
    assert bad.size == 0, [(int(b) // 128, int(b) % 128) for b in bad[:8]]          # (slot, word)
    assert int(host(fixed)[0]) == want_fixed
    assert want_fixed == 8 * (128 - 16)                                               # every word that is no code word counts once


# ------------------------------------------------------------------ config 2: RX demod (FFT + demap)
@pytest.mark.parametrize("n,mod,guard,nsym", [(64, 6, True, 320), (64, 2, False, 64), (64, 1, True, 40),
                                              (128, 4, True, 33), (1024, 6, True, 12), (4096, 8, True, 5),
                                              (512, 8, False, 9)])
def test_rx_demod(api, orc, n, mod, guard, nsym):
    rng = np.random.default_rng(1000 + n + mod)
    x, data = make_symbols(orc, rng, nsym, n, guard, mod, snr_db=32.0)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    S = n + n // 4
    # as one "frame" holding nsym symbols, and as nsym/ k frames of k symbols
    out, soft = ctx.rx_demod(dev(ctx, x).reshape(1, -1), syms_per_frame=nsym, want_soft=True)
    want, wsoft = orc.rx_demod(wide(x), n, guard, mod, want_soft=True)
    assert rel_err(host(soft), wsoft) <= TOL
    excused = assert_bytes_match(bytes(host(out).ravel()), want, wsoft, mod, what=f"rx_demod n={n}")
    assert excused == 0
    assert want == data  # 32 dB: error free, so decoded BER is identical (0) on both sides
    k = 4 if nsym % 4 == 0 else 1
    out2 = ctx.rx_demod(dev(ctx, x).reshape(nsym // k, k * S), syms_per_frame=k)
    assert bytes(host(out2).ravel()) == bytes(host(out).ravel())


@pytest.mark.parametrize("hk_on", [False, True])
@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_rx_demod_fast64_every_instantiation(api, orc, mod, guard, hk_on):
    """Every k_demod64<BPS, GUARD, HK> that run_demod64_fast (kernels_n64.hip) can dispatch, reached the way the headline
    does (no soft output, syms_per_frame % 8 == 0) and compared DIRECTLY with the oracle's bytes: 8, 16 and 24 symbols
    per frame (groups_per_frame 1, 2, 3: the blk_/step_ frame-advance arithmetic) over the same samples, many workgroups,
    and for three of the combinations enough groups (> 8192 = 256 CUs x 8 workgroups x 4 waves) that the persistent grid
    wraps.  src/receiver.rs:99-190."""
    big = (mod, guard, hk_on) in ((6, True, False), (6, True, True), (2, False, False))
    frames24 = 2752 if big else 1032            # frames of 24 symbols; x3 / x1.5 frames of 8 / 16 (8256 / 3096 groups: store bursts of 16 / 8)
    nsym = frames24 * 24
    rng = np.random.default_rng(4000 + 10 * mod + 2 * guard + hk_on)
    x, data = make_symbols_np(orc, rng, nsym, 64, guard, mod, snr_db=34.0)
    ctx = api.Context(n_fft=64, modulation=mod, guard_bands=guard)
    hk = fc32(1.0 + 0.2 * (rng.standard_normal(64) + 1j * rng.standard_normal(64))) if hk_on else None
    want, wsoft = orc.rx_demod(wide(x), 64, guard, mod, hk=None if hk is None else wide(hk), want_soft=True)
    if not hk_on:
        assert want == data                     # 34 dB, H == 1: error free on the oracle side
    xd = dev(ctx, x)
    hkd = None if hk is None else dev(ctx, hk)
    for k in (8, 16, 24):
        out = ctx.rx_demod(xd.reshape(nsym // k, k * 80), syms_per_frame=k, hk=hkd)   # no soft -> k_demod64
        # the kernel that ran, not only the bytes: the launcher falls back to the generic k_sym outside its envelope
        want_kernel = "k_demod64<burst%d>" % (16 if nsym // 8 % 16 == 0 else 8 if nsym // 8 % 8 == 0 else 4) if (mod, guard, hk_on) == (6, True, False) else "k_demod64"
        assert ctx.last_dispatch() == want_kernel, (ctx.last_dispatch(), k)
        excused = assert_bytes_match(bytes(host(out).ravel()), want, wsoft, mod, what=f"k_demod64<{mod},{guard},{hk_on}> k={k}")
        assert excused <= 2
    # first_symbol > 0 and a frame stride larger than the frame: symbols 8..15 of 24-symbol frames
    out = ctx.rx_demod(xd.reshape(frames24, 24 * 80), syms_per_frame=8, first_symbol=8, hk=hkd)
    assert ctx.last_dispatch().startswith("k_demod64")
    bps = ctx.bytes_per_symbol
    wsel = np.frombuffer(want, np.uint8).reshape(frames24, 24 * bps)[:, 8 * bps:16 * bps]
    ssel = np.asarray(wsoft).reshape(frames24, 24, -1)[:, 8:16].reshape(-1)
    assert_bytes_match(bytes(host(out).ravel()), bytes(wsel.ravel()), ssel, mod, what="first_symbol=8")


@pytest.mark.parametrize("mod,guard,per_frame_hk", [(8, True, False), (6, True, True), (2, False, False)])
def test_rx_demod_4096_many_symbols_per_frame(api, orc, mod, guard, per_frame_hk):
    """k_demod4096 (config 5 RX) against the oracle directly, with 11 symbols per frame and 3 frames (33 symbols:
    the prefetch pipeline runs deeper than its warm-up, a frame boundary falls inside it), shared / per-frame / no
    channel.  src/receiver.rs:99-190."""
    n, k, nf = 4096, 11, 3
    rng = np.random.default_rng(4096 + mod)
    x, data = make_symbols_np(orc, rng, k * nf, n, guard, mod, snr_db=36.0)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    xs = x.reshape(nf, k * 5120)
    hks = fc32(1.0 + 0.2 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))))
    if mod == 2:
        out = host(ctx.rx_demod(dev(ctx, xs), k))
        assert ctx.last_dispatch() == "k_demod4096"
        want, wsoft = orc.rx_demod(wide(x), n, guard, mod, want_soft=True)
        assert want == data
        assert_bytes_match(bytes(out.ravel()), want, wsoft, mod, what="k_demod4096 H=1")
        return
    hk_dev = dev(ctx, hks if per_frame_hk else hks[0])
    out = host(ctx.rx_demod(dev(ctx, xs), k, hk=hk_dev))
    assert ctx.last_dispatch() == "k_demod4096"
    for f in range(nf):
        want, wsoft = orc.rx_demod(wide(xs[f]), n, guard, mod, hk=wide(hks[f if per_frame_hk else 0]), want_soft=True)
        assert_bytes_match(bytes(out[f]), want, wsoft, mod, what=f"k_demod4096 frame {f}")


@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("n", [128, 256, 512, 1024, 2048])
def test_rx_demod_mid_every_instantiation(api, orc, n, guard):
    """k_demod_mid<R, BPS, GUARD> (kernels_mid.hip, N = 64 R) against the oracle for every modulation, 11 symbols per frame
    (frame boundaries fall inside a workgroup step), no / shared / per-frame channel, on a 3-workgroup grid so that every
    workgroup runs several steps of the prefetch and deferred-store pipeline; every call asserts that k_demod_mid served it
    (ofdm_last_dispatch), not the generic fallback.  src/receiver.rs:99-190."""
    k = 11
    nf = max(3, -(-7 * (32 // (n // 64)) // k))
    S = n + n // 4
    for mod in (1, 2, 4, 6, 8):
        rng = np.random.default_rng(n * 10 + mod)
        x, data = make_symbols_np(orc, rng, k * nf, n, guard, mod, snr_db=38.0)
        ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 3})
        xs = x.reshape(nf, k * S)
        out = host(ctx.rx_demod(dev(ctx, xs), k))
        assert ctx.last_dispatch() == "k_demod_mid"
        want, wsoft = orc.rx_demod(wide(x), n, guard, mod, want_soft=True)
        assert want == data
        assert_bytes_match(bytes(out.ravel()), want, wsoft, mod, what=f"k_demod_mid<{n // 64},{mod},{guard}> H=1")
        hks = fc32(1.0 + 0.2 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))))
        for per_frame in (False, True):
            out = host(ctx.rx_demod(dev(ctx, xs), k, hk=dev(ctx, hks if per_frame else hks[0])))
            assert ctx.last_dispatch() == "k_demod_mid"
            for f in (0, nf // 2, nf - 1):
                want, wsoft = orc.rx_demod(wide(xs[f]), n, guard, mod, hk=wide(hks[f if per_frame else 0]), want_soft=True)
                assert_bytes_match(bytes(out[f]), want, wsoft, mod, what=f"k_demod_mid<{n // 64},{mod},{guard}> frame {f}")
        # first_symbol > 0 on a stride larger than the part demodulated
        out = host(ctx.rx_demod(dev(ctx, xs), 4, first_symbol=5))
        assert ctx.last_dispatch() == "k_demod_mid"
        want, wsoft = orc.rx_demod(wide(x), n, guard, mod, want_soft=True)
        bps = ctx.bytes_per_symbol
        wsel = np.frombuffer(want, np.uint8).reshape(nf, k * bps)[:, 5 * bps:9 * bps]
        ssel = np.asarray(wsoft).reshape(nf, k, -1)[:, 5:9].reshape(-1)
        assert_bytes_match(bytes(out.ravel()), bytes(wsel.ravel()), ssel, mod, what="first_symbol=5")


@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_tx_symbols_mid_every_instantiation(api, orc, n, guard):
    """k_tx_mid<R, GUARD> (kernels_mid.hip) and k_tx4096<GUARD> (kernels_n4096.hip) against the oracle's modulate + encode_block +
    prefix_block for every modulation: a stream that ends inside a symbol, pilot-only symbols behind it, a 2-workgroup grid
    (>= 4 steps of the byte-prefetch pipeline per workgroup).  src/transmitter.rs:40-53, 108-181."""
    import torch
    G = max(1, 32 // (n // 64))
    n_sym = 5 * G + 3
    for mod in (1, 2, 4, 6, 8):
        rng = np.random.default_rng(n * 7 + mod)
        ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 2})
        bps, nd = ctx.bytes_per_symbol, ctx.data_carriers
        nb = (n_sym - 3) * bps + bps // 3 + 1          # the last byte-carrying symbol is partly filled, two carry only pilots
        data = rng.integers(0, 256, nb, dtype=np.uint8)
        fused = host(ctx.tx_symbols(torch.from_numpy(data.copy()).to(ctx.device), n_sym=n_sym))
        # the stream kernels stage a symbol's bytes as whole dwords: the one shape with 6-byte symbols (N = 64, BPSK, guard bands)
        # is outside their envelope and is served -- and checked here -- through the generic kernel
        assert ctx.last_dispatch() == ("k_sym<tx>" if bps % 4 else "k_tx4096" if n == 4096 else "k_tx_mid"), (ctx.last_dispatch(), n, mod)
        opts = np.asarray(orc.modulate(bytes(data), mod))
        pts = np.zeros(n_sym * nd, np.complex128)
        pts[: opts.size] = opts
        want = np.stack([orc.prefix_block(orc.encode_block(pts[i * nd:(i + 1) * nd], n, guard)[0]) for i in range(n_sym)])
        assert rel_err(fused, want) < TOL, (n, mod, guard)
        # per symbol as well: a misplaced symbol or prefix would hide in the global norm of a long stream
        for i in (0, 1, G, n_sym - 3, n_sym - 1):
            assert rel_err(fused[i], want[i]) < 4 * TOL, (n, mod, guard, i)


@pytest.mark.parametrize("n,mod,guard", [(128, 6, True), (256, 2, False), (512, 8, True), (1024, 4, True), (2048, 6, False),
                                         (4096, 8, True), (4096, 6, False)])
def test_rx_demod_mid_frame_mode(api, orc, n, mod, guard):
    """k_demod_mid<..., FRAME = true> / k_demod4096<..., FRAME = true>: what the decode chain asks of the demodulator after timing (src/receiver.rs:20-83) --
    a per-frame start offset, CFO derotation with sample ids counted from that start, a per-frame channel, and zero-fill past
    the end of the capture (pad_chunk, receiver.rs:203-210) -- against the oracle, frame by frame, on a 3-workgroup grid."""
    import torch
    rng = np.random.default_rng(n + mod)
    S, k, nf = n + n // 4, 7, 6
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 3})
    x, _ = make_symbols_np(orc, rng, k * nf, n, guard, mod, snr_db=38.0)
    x = wide(x).reshape(nf, k * S)
    offs = rng.integers(0, 97, nf).astype(np.int32)
    fds = (rng.random(nf) * 1.8 - 0.9) * np.pi / S
    span = k * S + 96
    frames = np.zeros((nf, span), np.complex128)
    for f in range(nf):
        # the transmitter's samples, shifted by the frame's offset and rotated by +f_delta (src/channel.rs:58-62: exp(+j f (i + 1)))
        frames[f, offs[f]:offs[f] + k * S] = x[f] * np.exp(1j * fds[f] * (np.arange(k * S) + 1))
    hks = fc32(1.0 + 0.2 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))))
    cut = span - (S // 2 + 13)   # the capture ends inside the last symbol of the frames with the largest offsets
    out = host(ctx.rx_demod(dev(ctx, fc32(frames)), k, offset=torch.from_numpy(offs).to(ctx.device),
                            f_delta=torch.from_numpy(fds).to(ctx.device), hk=dev(ctx, hks), frame_len=cut))
    assert ctx.last_dispatch() == ("k_demod4096<frame>" if n == 4096 else "k_demod_mid<frame>")
    for f in range(nf):
        seg = wide(fc32(frames[f]))[: cut][offs[f]:]
        seg = np.concatenate([seg, np.zeros(max(0, k * S - seg.size), np.complex128)])[: k * S]
        seg = orc.cfo_rotate(seg, fds[f], 0)
        want, wsoft = orc.rx_demod(seg, n, guard, mod, hk=wide(hks[f]), want_soft=True)
        assert_bytes_match(bytes(out[f]), want, wsoft, mod, what=f"frame mode n={n} frame {f}")


def test_rx_demod_with_channel_and_tail_padding(api, orc):
    rng = np.random.default_rng(77)
    n, mod = 64, 6
    x, data = make_symbols(orc, rng, 16, n, True, mod, snr_db=35.0)
    hk = fc32(1.0 + 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True)
    out, soft = ctx.rx_demod(dev(ctx, x).reshape(1, -1), 16, hk=dev(ctx, hk), want_soft=True)
    want, wsoft = orc.rx_demod(wide(x), n, True, mod, hk=wide(hk), want_soft=True)
    assert rel_err(host(soft), wsoft) <= TOL
    assert_bytes_match(bytes(host(out).ravel()), want, wsoft, mod, what="rx_demod hk")
    # frame_len shorter than the symbols asked for: missing samples read as zero (pad_chunk, receiver.rs:203-210)
    cut = 15 * 80 + 30
    xp = np.concatenate([x[:cut], np.zeros(16 * 80 - cut, np.complex64)])
    out_p = ctx.rx_demod(dev(ctx, x).reshape(1, -1), 16, frame_len=cut)
    assert bytes(host(out_p).ravel()) == orc.rx_demod(wide(xp), n, True, mod)


@pytest.mark.parametrize("n,mod,guard", [(4096, 4, True), (4096, 6, False), (64, 4, True), (1024, 6, True)])
def test_rx_demod_equalised_fast_kernels(api, orc, n, mod, guard):
    """rx_demod with a channel (equalise, receiver.rs:68-70) through the shape-specialised kernels (k_demod64 with a shared
    channel, k_demod4096 with a shared and a per-frame channel) and the generic one (N = 1024), without soft output so
    that the fast paths are taken: bytes against the oracle's, differing decisions excused only at a boundary."""
    rng = np.random.default_rng(n + mod)
    nsym = 8 if n == 64 else 3
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    S = ctx.S
    frames, wants, softs, hks = [], [], [], []
    for f in range(2):
        x, _ = make_symbols(orc, rng, nsym, n, guard, mod, snr_db=33.0)
        hk = fc32(1.0 + 0.25 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
        frames.append(x); hks.append(hk)
    xs = np.stack(frames)
    # shared channel
    out = host(ctx.rx_demod(dev(ctx, xs), nsym, hk=dev(ctx, hks[0])))
    for f in range(2):
        want, wsoft = orc.rx_demod(wide(xs[f]), n, guard, mod, hk=wide(hks[0]), want_soft=True)
        assert_bytes_match(bytes(out[f]), want, wsoft, mod, what=f"shared hk, frame {f}")
    # one channel per frame
    out = host(ctx.rx_demod(dev(ctx, xs), nsym, hk=dev(ctx, np.stack(hks))))
    for f in range(2):
        want, wsoft = orc.rx_demod(wide(xs[f]), n, guard, mod, hk=wide(hks[f]), want_soft=True)
        assert_bytes_match(bytes(out[f]), want, wsoft, mod, what=f"per-frame hk, frame {f}")


# ------------------------------------------------------------------ EXT-3: Schmidl-Cox, a14, a15, a16
# N = 64 searches with W = 3 L go through k_sc80 (every lag on f64 prefix differences, kernels_sc80.hip); the round-4 f32 filter pair
# (k_sc_cf) stays in the library for other windows, for the one-pass receive kernel and as the A/B: both are held to the oracle
SC_DETECTORS = [pytest.param({}, id="k_sc80"), pytest.param({"no_sc80": 1}, id="k_sc_cf")]


@pytest.mark.parametrize("sc_tuning", SC_DETECTORS)
def test_sc_correlate_batch(api, orc, sc_tuning):
    rng = np.random.default_rng(5)
    nfr, span = 48, 2176
    caps, delays, fds = [], [], []
    for f in range(nfr):
        d = int(rng.integers(1, 65))
        fd = (rng.random() * 1.9 - 0.95) * np.pi / 80
        payload = bytes(rng.integers(0, 256, 560, dtype=np.uint8))
        c, _ = make_capture(orc, rng, orc.QAM64, True, payload, span, d, fd)
        caps.append(c); delays.append(d); fds.append(fd)
    caps = np.stack(caps)
    caps[7] = 0  # nothing to find
    caps[8] = fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))  # noise only
    ctx = api.Context(modulation=api.QAM64, guard_bands=True, tuning=sc_tuning)
    d_hat, f_delta, metric = ctx.sc_correlate(dev(ctx, caps))
    assert ("k_sc80" in ctx.last_dispatch()) == (not sc_tuning) and ("k_sc_cf" in ctx.last_dispatch()) == bool(sc_tuning), ctx.last_dispatch()
    d_hat, f_delta, metric = host(d_hat), host(f_delta), host(metric)
    for f in range(nfr):
        wd, wp, wm, wfd = orc.sc_sync(wide(caps[f]), 80, 3, 0, 0.5)
        assert d_hat[f] == wd, f"frame {f}"
        if wd >= 0:
            assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6
            if f not in (7, 8):
                assert wd == delays[f] + 80 + 9 and abs(wfd - fds[f]) < 2e-4
    assert d_hat[7] == -1 and d_hat[8] == -1
    # bounded search and a non-default stride / frame_len
    d2, _, _ = ctx.sc_correlate(dev(ctx, caps), frame_len=2000, n_lags=256)
    for f in range(0, nfr, 5):
        assert host(d2)[f] == orc.sc_sync(wide(caps[f][:2000]), 80, 3, 256, 0.5)[0]


@pytest.mark.parametrize("reps", [3, 1, 2])
def test_sc_correlate_two_launch_search_equals_the_whole_search(api, orc, reps):
    """N = 64 searches over many lags run as two launches (kernels_sync.hip, run_sc_fast): the first looks at the first
    `sc_first_lags` lags only and lists every frame those lags do not DETERMINE (no crossing among them, or a peak window that
    reaches beyond them), the second is the whole search over that list.  Packets whose crossing lies well inside, just inside
    (window cut by the boundary), on and beyond the first lags, noise-only and empty slots, on a capped grid (the list is walked
    by a persistent grid): every result bit-identical to the single-launch search, and to the oracle's."""
    rng = np.random.default_rng(77 + reps)
    span, firsts = 2400, (384, 300, 900)
    payload = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    delays = [1, 40, 64, 100, 110, 118, 119, 120, 121, 130, 200, 206, 207, 208, 209, 250, 359, 360, 361, 700, 810, 811, 812, 1500, 1790, 2000]
    caps = []
    for d in delays:   # the crossing sits at about d + 80 + 9 - W .. : delays chosen around first - W - 89 for each `first`
        c, _ = make_capture(orc, rng, orc.QAM64, True, payload, span, d, (rng.random() * 1.9 - 0.95) * np.pi / 80)
        caps.append(c)
    caps.append(np.zeros(span, np.complex64))
    caps.append(fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))))
    caps = np.stack(caps * 3)   # 81 frames: more than the capped grid
    want = [orc.sc_sync(wide(c), 80, reps, 0, 0.5) for c in caps[: len(delays) + 2]]
    ref = None
    for first in (0,) + firsts:
        ctx = api.Context(modulation=api.QAM64, guard_bands=True, sync_window_reps=reps, tuning={"sc_first_lags": first, "grid_cap": 5, "no_sc80": 1})
        d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
        disp = ctx.last_dispatch()
        assert ("k_sc_cf<128,first>+k_sc_cf<256,list>" in disp) == (first > 0), disp
        if ref is None:
            ref = (d_hat, f_delta, metric)
            for f, (wd, _, wm, wfd) in enumerate(want):
                assert d_hat[f] == wd, f"frame {f}"
                if wd >= 0:
                    assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6
            assert int((d_hat[: len(delays)] >= 0).sum()) >= len(delays) - 2 and d_hat[len(delays)] == -1
        else:
            assert (d_hat == ref[0]).all() and (f_delta == ref[1]).all() and (metric == ref[2]).all(), f"first = {first}"
    # the decode chain takes the same path
    res = []
    for first in (0, 384, 576):
        ctx = api.Context(modulation=api.QAM64, guard_bands=True, sync_window_reps=reps, tuning={"sc_first_lags": first, "no_sc80": 1})
        r = ctx.decode_batch(dev(ctx, caps), max_symbols=8)
        assert ("k_sc_cf<128,first>+k_sc_cf<256,list>" in ctx.last_dispatch()) == (first > 0), ctx.last_dispatch()
        res.append({k: host(v) for k, v in r.items()})
    # ... and the exact streaming detector (the default for W = 3 L), on a capped grid: the same decisions, sums equal to rounding
    ctx = api.Context(modulation=api.QAM64, guard_bands=True, sync_window_reps=reps, tuning={"grid_cap": 3})
    d80, f80, m80 = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
    assert ("k_sc80" in ctx.last_dispatch()) == (reps == 3), ctx.last_dispatch()
    assert (d80 == ref[0]).all() and np.abs(f80 - ref[1]).max() <= 1e-12 and np.abs(m80 - ref[2]).max() <= 1e-6
    r = ctx.decode_batch(dev(ctx, caps), max_symbols=8)
    res.append({k: host(v) for k, v in r.items()})
    for other in res[1:]:
        for k in ("status", "offset", "len"):
            assert (res[0][k] == other[k]).all(), k
        assert np.abs(res[0]["f_delta"] - other["f_delta"]).max() <= 1e-12
        for f in range(caps.shape[0]):   # rows are defined up to the frame's length only
            assert (res[0]["bytes"][f, : res[0]["len"][f]] == other["bytes"][f, : other["len"][f]]).all(), f
    assert int((res[0]["status"][:20] == 0).sum()) >= 18


def test_sc_first_lags_at_the_edge_of_the_first_tile(api, orc):
    """with sc_first_lags in 949 .. 1280 the first launch's stage (first + W + L + 11 samples) would not fit its
    128-chunk tile of 1280 samples; such values take the single-launch search, the largest that fits (948 for W = 240) is clamped
    to the tile, values above 1280 are refused -- and every accepted value gives the whole search's results."""
    rng = np.random.default_rng(949)
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64)
    span = 2544   # 2225 lags: the most a one-tile search holds is 2240 (256 chunks - W - L)
    caps = np.stack([through_channel(orc, rng, tx, span, d, 0.01, 30.0) for d in (5, 380, 400, 330, 270, 410)])
    want = [orc.sc_sync(wide(c), 80, 3, 0, 0.5) for c in caps]
    for first, kernel in ((948, "k_sc_cf<128,first>"), (949, "k_sc_cf<256>"), (955, "k_sc_cf<256>"), (1280, "k_sc_cf<256>")):
        ctx = api.Context(modulation=api.QAM64, guard_bands=True, tuning={"sc_first_lags": first, "no_sc80": 1})
        d, fd, m = ctx.sc_correlate(dev(ctx, caps))
        assert kernel in ctx.last_dispatch(), (first, ctx.last_dispatch())
        for f, (wd, _, wm, wfd) in enumerate(want):
            assert int(host(d)[f]) == wd and abs(float(host(fd)[f]) - wfd) <= 1e-9, (first, f)
    ctx = api.Context(modulation=api.QAM64, guard_bands=True)
    for key, bad in (("sc_first_lags", 1281), ("tx_waves", 0), ("tx_waves", 33), ("demod64_burst", 5), ("sc_wg_per_cu", 17)):
        with pytest.raises(api.OfdmError):
            ctx.set_tuning(key, bad)


def test_sc80_streaming_detector_corner_cases(api, orc):
    """k_sc80 (kernels_sc80.hip) on what its design has to get right: batches that do not fill the last wavefront's four rows, a
    capped grid walking many groups, bounded searches and captures barely longer than one window (the stream is clamped at the
    last sample a lag reads), thresholds that are not a power of two (the crossing filter's fused compare), all-zero lead-ins
    (exact prefix differences: no slow list), and captures whose dynamic range defeats prefix differences -- an exact-zero gap
    behind a burst, a packet 75 dB below a burst -- which must come back from the slow list with the oracle's answer."""
    ordinary, dynamic = sc80_corner_captures(orc)
    # (a) ragged batches, capped grid, bounded and short searches, other thresholds
    for nfr in (1, 2, 3, 5, 13):
        caps = np.stack(ordinary[:nfr])
        for thr, n_lags, flen in SC80_SEARCHES:
            ctx = api.Context(modulation=api.QAM64, guard_bands=True, sync_threshold=thr, tuning={"grid_cap": 2})
            d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps), frame_len=flen, n_lags=n_lags))
            assert ctx.last_dispatch().startswith("k_sc80"), ctx.last_dispatch()
            for f in range(nfr):
                wd, _, wm, wfd = orc.sc_sync(wide(caps[f][:flen]), 80, 3, n_lags, thr)
                assert d_hat[f] == wd, (nfr, thr, n_lags, flen, f, int(d_hat[f]), wd)
                if wd >= 0:
                    assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6, (nfr, thr, n_lags, flen, f)
    # (b) dynamic range
    caps, lead = dynamic, dynamic[0]
    ctx = api.Context(modulation=api.QAM64, guard_bands=True)
    d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps[:1])))
    assert ctx.get_tuning("stat_sc_slow_frames") == 0 and d_hat[0] == orc.sc_sync(wide(lead), 80, 3, 0, 0.5)[0] >= 0
    d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
    slow = ctx.get_tuning("stat_sc_slow_frames")
    assert 2 <= slow <= 3, slow                                                   # the gap and the quiet packet (the hot one may or may not be trusted)
    for f in range(caps.shape[0]):
        wd, _, wm, wfd = orc.sc_sync(wide(caps[f]), 80, 3, 0, 0.5)
        assert d_hat[f] == wd, (f, int(d_hat[f]), wd)
        if wd >= 0:
            assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6 * max(1.0, wm), f


@pytest.mark.parametrize("n", [64, 256, 1024])
def test_streaming_detectors_on_rows_of_any_alignment(api, orc, n):
    """LDS-DMA takes any 4-byte aligned source (tools/lab/glds_align.hip), so k_sc80 / k_sc_stream / k_rxframe1024 no longer ask for
    16-byte aligned rows and even strides (round 4 sent such batches to the two-pass / one-tile kernels, 2-5 x slower): a batch whose
    base is 8 bytes off a 16-byte boundary with an ODD row stride -- every other row misaligned -- against the same captures in an
    aligned buffer and against the oracle; the decode chain on the same rows."""
    import torch
    rng = np.random.default_rng(900 + n)
    mod, guard = api.QAM16, True
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    S = ctx.S
    nbytes = 3 * ctx.bytes_per_symbol - 16
    D = ctx.data_symbols(nbytes)
    span = (ctx.frame_samples(nbytes) + S + 40) // 2 * 2
    nfr = 9
    caps, pays = [], []
    for f in range(nfr):
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        tx = orc.encode(pay, guard, mod, n)
        caps.append(through_channel(orc, rng, tx, span, int(rng.integers(1, S)), (rng.random() * 1.6 - 0.8) * np.pi / S, 35.0, data_start=10 * S))
        pays.append(pay)
    caps[4] = fc32(0.004 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))
    caps = np.stack(caps)
    stride = span + 1
    buf = torch.zeros(nfr * stride + 2, dtype=torch.complex64, device=ctx.device)
    rows = buf[1:1 + nfr * stride].view(nfr, stride)                    # contiguous rows of span + 1 samples, the last one unused
    rows[:, :span].copy_(torch.from_numpy(caps).to(ctx.device))
    assert rows.data_ptr() % 16 == 8 and rows.stride(0) % 2 == 1
    want_search = "k_sc80" if n == 64 else "k_sc_stream"
    da, fa, ma = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
    assert ctx.last_dispatch().startswith(want_search), ctx.last_dispatch()
    db, fb, mb = (host(t) for t in ctx.sc_correlate(rows, frame_len=span))
    assert ctx.last_dispatch().startswith(want_search), ctx.last_dispatch()
    assert np.array_equal(da, db) and np.array_equal(fa, fb) and np.array_equal(ma, mb)
    for f in range(nfr):
        wd, _, wm, wfd = orc.sc_sync(wide(caps[f]), S, 3, 0, 0.5)
        assert db[f] == wd and (wd < 0 or (abs(fb[f] - wfd) <= 1e-9 and abs(mb[f] - wm) <= 1e-6)), f
    ra = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D).items()}
    rb = {k: host(v) for k, v in ctx.decode_batch(rows, max_symbols=D, frame_len=span).items()}
    disp = ctx.last_dispatch()
    assert disp.startswith(want_search) and (n != 1024 or "k_rxframe1024<finish>" in disp), disp
    for k in ("status", "len"):
        assert np.array_equal(ra[k], rb[k]), k
    good = [f for f in range(nfr) if f != 4]
    assert np.array_equal(ra["offset"][good], rb["offset"][good]) and np.array_equal(ra["f_delta"][good], rb["f_delta"][good])
    assert all(np.array_equal(ra["bytes"][f][: ra["len"][f]], rb["bytes"][f][: rb["len"][f]]) for f in good)
    assert (rb["status"][good] == 0).all() and rb["status"][4] != 0
    for f in good:   # (the FIR channel's weak bins leave a stray byte error at 35 dB; parity with the oracle is the other tests' subject)
        got = bytes(rb["bytes"][f][: rb["len"][f]])
        assert len(got) == nbytes and sum(a != b for a, b in zip(got, pays[f])) <= 3, f
    # odd slot lengths: with slack behind every row (stride = length + 1) and as tight rows (stride = length: k_sc80 takes all rows but
    # the last, whose "one sample past the slot" would lie outside the batch)
    odd = span - 1
    want = [orc.sc_sync(wide(caps[f][:odd]), S, 3, 0, 0.5) for f in range(nfr)]
    tight = torch.from_numpy(np.ascontiguousarray(caps[:, :odd])).to(ctx.device)
    for x, flen, label in ((dev(ctx, caps), odd, "slack"), (tight, None, "tight")):
        d, fdl, m = (host(t) for t in ctx.sc_correlate(x, frame_len=flen))
        assert ctx.last_dispatch().startswith(want_search), (label, ctx.last_dispatch())
        for f in range(nfr):
            wd, _, wm, wfd = want[f]
            assert d[f] == wd and (wd < 0 or (abs(fdl[f] - wfd) <= 1e-9 and abs(m[f] - wm) <= 1e-6)), (label, f)


def test_sc80_on_slots_longer_than_one_tile(api, orc):
    """N = 64 slots of more than 2 560 samples (BPSK frames of more than ~110 payload bytes: the reference's own modulation) used to
    fall to the general multi-tile search, 12 x slower per byte; k_sc80 streams a slot of any length, so a batch of at least 512 such
    slots takes it.  Packets early, late (crossing beyond the first 2 560 lags) and absent; a burst in front of a packet 75 dB down
    sends frames to the slow list, which for more lags than one k_sc_tile tile is redone in three launches (first crossing per tile,
    earliest per frame, peak window).  Every frame against the generic search (lab key no_sc80), a sample against the oracle; a
    batch of 64 such slots keeps the multi-tile search (one row per frame would leave the chip empty)."""
    rng = np.random.default_rng(8080)
    tx = orc.encode(bytes(rng.integers(0, 256, 300, dtype=np.uint8)), True, orc.BPSK)
    assert tx.size == 63 * 80
    span, nfr = 9000, 520
    caps = np.zeros((nfr, span), np.complex64)
    kinds = []
    for f in range(nfr):
        kind = f % 5
        if kind == 4:                                     # noise only
            caps[f] = fc32(0.004 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))
        else:
            d = int(rng.integers(1, 200)) if kind < 2 else int(rng.integers(2700, 3600))
            caps[f] = through_channel(orc, rng, tx, span, d, float((rng.random() * 1.9 - 0.95) * np.pi / 80), 30.0)
            if kind == 1 or kind == 3:                    # burst, then the packet 75 dB down: prefix differences are not trusted
                w = 1e-3 * wide(caps[f])
                w[5:25] += 3.0 * (rng.standard_normal(20) + 1j * rng.standard_normal(20))
                caps[f] = fc32(w)
        kinds.append(kind)
    a = api.Context(modulation=api.BPSK, guard_bands=True, tuning={"grid_cap": 24})
    b = api.Context(modulation=api.BPSK, guard_bands=True, tuning={"no_sc80": 1})
    x = dev(a, caps)
    da, fa, ma = (host(t) for t in a.sc_correlate(x))
    assert a.last_dispatch() == "k_sc80+k_sc_tile<list,cross>+k_sc_tile<list,peak>", a.last_dispatch()
    slow = a.get_tuning("stat_sc_slow_frames")
    assert 100 <= slow <= 2 * (nfr // 5) + 8, slow
    db, fb, mb = (host(t) for t in b.sc_correlate(dev(b, caps)))
    assert b.last_dispatch().startswith("k_sc_tile<cross>"), b.last_dispatch()
    assert np.array_equal(da, db)
    found = da >= 0
    assert found.sum() >= 4 * (nfr // 5) - 2 and (da[np.array(kinds) == 4] == -1).all()
    assert np.abs(fa[found] - fb[found]).max() <= 1e-12 and np.abs(ma[found] - mb[found]).max() <= 1e-6
    assert (da[np.array(kinds) >= 2][da[np.array(kinds) >= 2] >= 0] > 2560).all()          # the late packets' crossings lie in the second tile
    for f in list(range(10)) + [nfr - 3, nfr - 2, nfr - 1]:
        wd, _, wm, wfd = orc.sc_sync(wide(caps[f]), 80, 3, 0, 0.5)
        assert da[f] == wd, (f, kinds[f], int(da[f]), wd)
        if wd >= 0:
            assert abs(fa[f] - wfd) <= 1e-9 and abs(ma[f] - wm) <= 1e-6 * max(1.0, wm), f
    # few long slots: the chip-wide multi-tile search stays
    d64 = host(a.sc_correlate(dev(a, caps[:64]))[0])
    assert a.last_dispatch().startswith("k_sc_tile<cross>"), a.last_dispatch()
    assert np.array_equal(d64, da[:64])
    # and the decode chain on such a batch: payloads back (the clean early / late packets)
    r = a.decode_batch(x, max_symbols=53)
    assert "k_sc80" in a.last_dispatch()
    ln = host(r["len"])
    clean = [f for f in range(nfr) if kinds[f] in (0, 2)]
    assert (ln[clean] == 300).all()


@pytest.mark.parametrize("sc_tuning", SC_DETECTORS)
def test_sc_correlate_untrusted_f32_filter(api, orc, sc_tuning):
    # A strong burst ahead of the frame makes the prefix energy >> window energy, so the fast kernel's f32 filter must
    # not be trusted there: those frames are redone by the all-f64 kernel (device-side slow list).  Results still exact.
    rng = np.random.default_rng(12)
    caps = []
    for f in range(24):
        payload = bytes(rng.integers(0, 256, 560, dtype=np.uint8))
        c, _ = make_capture(orc, rng, orc.QAM64, True, payload, 2176, int(rng.integers(20, 60)), 0.01, 30.0)
        c = c.copy()
        if f % 2 == 0:
            c[2:14] += fc32(40.0 * (rng.standard_normal(12) + 1j * rng.standard_normal(12)))
        caps.append(c)
    caps = np.stack(caps)
    ctx = api.Context(modulation=api.QAM64, guard_bands=True, tuning=sc_tuning)
    d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
    for f in range(24):
        wd, _, wm, wfd = orc.sc_sync(wide(caps[f]), 80, 3, 0, 0.5)
        assert d_hat[f] == wd and abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6, f"frame {f}"


@pytest.mark.parametrize("sc_tuning", SC_DETECTORS)
def test_sc_correlate_coarse_fine_corner_cases(api, orc, sc_tuning):
    """The coarse-then-fine filter's less-travelled paths, against the f64 oracle on synthetic period-80 signals:
    false alarms (a flagged chunk whose 320-lag group holds no crossing), a metric that creeps up so that the crossing
    lies late in its group (restart at the crossing's chunk), frames that are periodic everywhere (every chunk
    flagged), plateaus (many equal maxima), packets at the very end of the searched lags, and pure tones."""
    rng = np.random.default_rng(2024)
    span, L = 2176, 80
    n = np.arange(span)

    def noise(sig):
        return sig * (rng.standard_normal(span) + 1j * rng.standard_normal(span))

    def periodic(start, stop, amp, seed_len=L):
        base = rng.standard_normal(seed_len) + 1j * rng.standard_normal(seed_len)
        x = np.zeros(span, complex)
        x[start:stop] = amp * np.resize(base, stop - start)
        return x

    caps = []
    for k in range(96):
        kind = k % 8
        if kind == 0:    # short periodic burst (M rises but stays < 0.5 or barely crosses), real header much later
            x = noise(0.3) + periodic(100, 100 + int(rng.integers(200, 330)), 0.45) + periodic(int(rng.integers(900, 1400)), span, 1.0)
        elif kind == 1:  # slowly growing periodic amplitude: the bound is exceeded long before the metric crosses
            ramp = np.clip((n - 200) / float(rng.integers(600, 1500)), 0, 1)
            x = noise(0.5) + ramp * periodic(0, span, 1.0)
        elif kind == 2:  # periodic everywhere, little noise: every chunk flagged, plateau of near-equal maxima
            x = noise(10.0 ** -float(rng.integers(2, 5))) + periodic(0, span, 1.0)
        elif kind == 3:  # exactly periodic and noiseless from some point on: exact ties
            x = periodic(int(rng.integers(0, 700)), span, 1.0)
        elif kind == 4:  # header only near the end of the searched range
            x = noise(0.05) + periodic(int(rng.integers(1500, 1800)), span, 1.0)
        elif kind == 5:  # pure tone with a CFO-like rotation (period-80 up to a phase ramp)
            x = noise(0.02) + 0.7 * np.exp(1j * (0.013 * n + 0.4)) * (n > int(rng.integers(50, 900)))
        elif kind == 6:  # two packets of different strength
            x = noise(0.1) + periodic(150, 700, 0.35) + periodic(1100, 1900, 1.0)
        else:            # metric hovering around the threshold: periodic part and noise of similar power
            x = noise(float(rng.uniform(0.55, 0.8))) + periodic(int(rng.integers(0, 600)), span, 1.0)
        caps.append(fc32(x))
    caps = np.stack(caps)
    ctx = api.Context(modulation=api.QAM64, guard_bands=True, tuning=sc_tuning)
    for n_lags in (0, 1000):
        d_hat, f_delta, metric = (host(t) for t in ctx.sc_correlate(dev(ctx, caps), n_lags=n_lags))
        found = ties = 0
        for f in range(caps.shape[0]):
            wd, _, wm, wfd = orc.sc_sync(wide(caps[f]), L, 3, n_lags, 0.5)
            if d_hat[f] != wd:
                # Only excuse: a TIE below f64 resolution (noiseless periodic plateaus: the true metric is exactly equal
                # at many lags, and which of them an f64 evaluation ranks first depends on its summation order).  The
                # GPU's lag must then lie in the oracle's peak window and carry the oracle's maximum to 1e-12.
                m = orc.sc_metric(wide(caps[f]), L, 3, n_lags)
                m = m[0] if isinstance(m, tuple) else m
                d1 = int(np.argmax(m >= 0.5))
                assert f % 8 in (2, 3) and wd >= 0 and d1 <= d_hat[f] <= d1 + 3 * L, f"frame {f} (kind {f % 8}, n_lags {n_lags}): {d_hat[f]} != {wd}"
                assert abs(m[d_hat[f]] - wm) <= 1e-12 * wm, f"frame {f}: not a tie ({m[d_hat[f]]} vs {wm})"
                ties += 1
            if wd >= 0:
                found += 1
                assert abs(metric[f] - wm) <= 1e-6 * max(1.0, wm), f"frame {f}"
                if d_hat[f] == wd:
                    assert abs(f_delta[f] - wfd) <= 1e-9, f"frame {f}"
        assert found >= 60 and ties <= 24


def test_sc_correlate_randomised_stress(ofdm):
    """tools/sc_stress.py: 600 random captures (SNR -3..40 dB, any delay, CFO up to +-pi/80, truncated frames, second
    packets, interferers) x 4 search configurations, every timing index / CFO / metric against the f64 oracle."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for detector in ("k_sc80", "k_sc_cf"):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "sc_stress.py"), "600", "3", detector], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.count(" 0 mismatches") == 4, detector + r.stdout[-2000:] + r.stderr[-2000:]


def test_sc_correlate_long_capture_multi_tile(api, orc):
    # one long capture (jetson_rx style): the frame sits past several 2560-lag tiles, odd start
    rng = np.random.default_rng(6)
    payload = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    tx = orc.encode(payload, False, orc.QPSK)
    span, delay, fd = 20000, 9137, 0.011
    cap = through_channel(orc, rng, tx, span, delay, fd, 25.0)
    ctx = api.Context(modulation=api.QPSK)
    d_hat, f_delta, metric = ctx.sc_correlate(dev(ctx, cap).reshape(1, -1))
    wd, _, wm, wfd = orc.sc_sync(wide(cap), 80, 3, 0, 0.5)
    assert int(host(d_hat)[0]) == wd == delay + 89
    assert abs(float(host(f_delta)[0]) - wfd) <= 1e-9 and abs(float(host(metric)[0]) - wm) <= 1e-6


def test_frequency_correction_cfo_rotate_estimate_channel(api, orc):
    rng = np.random.default_rng(8)
    ctx = api.Context(modulation=api.QPSK)
    left = fc32(rng.standard_normal((6, 80)) + 1j * rng.standard_normal((6, 80)))
    fds = rng.random(6) * 0.03
    right = fc32(left * np.exp(1j * fds[:, None] * 80) + 0.01 * (rng.standard_normal((6, 80)) + 1j * rng.standard_normal((6, 80))))
    got = host(ctx.frequency_correction(dev(ctx, np.concatenate([left, right], axis=1))))
    for i in range(6):
        want = orc.frequency_correction(wide(left[i]), wide(right[i]))
        assert abs(got[i] - want) <= 1e-12  # f64 on both sides (CFO to 1e-9 or better)
    # CFO derotation with the f64-reduced phase: long frame, first_index offset
    x = fc32(rng.standard_normal((2, 5000)) + 1j * rng.standard_normal((2, 5000)))
    import torch
    fd = torch.tensor([0.0371, -0.0123], dtype=torch.float64, device=ctx.device)
    first = torch.tensor([0, 777], dtype=torch.int32, device=ctx.device)
    y = host(ctx.cfo_rotate(dev(ctx, x), fd, first))
    for r in range(2):
        assert rel_err(y[r], orc.cfo_rotate(wide(x[r]), float(fd[r]), int(first[r]))) <= TOL
    # estimate_channel on frames through the FIR channel (with offsets and CFO derotation)
    frames, offs, cf = [], [], []
    for f in range(5):
        payload = bytes(rng.integers(0, 256, 100, dtype=np.uint8))
        d, f_d = int(rng.integers(0, 30)), (rng.random() - 0.5) * 0.05
        cap, _ = make_capture(orc, rng, orc.QPSK, False, payload, 2000, d, f_d, 30.0)
        frames.append(cap); offs.append(d + 5); cf.append(f_d)
    frames = np.stack(frames)
    off_t = torch.tensor(offs, dtype=torch.int32, device=ctx.device)
    fd_t = torch.tensor(cf, dtype=torch.float64, device=ctx.device)
    hk = host(ctx.estimate_channel(dev(ctx, frames), off_t, fd_t))
    trn = orc.default_training(64)
    for f in range(5):
        seg = orc.cfo_rotate(wide(frames[f][offs[f]:]), cf[f], 0)
        want = orc.estimate_channel(seg[5 * 80:10 * 80], trn, 64)
        assert rel_err(hk[f], want) <= TOL


# ------------------------------------------------------------------ a1: encode (TX pipeline)
@pytest.mark.parametrize("n,mod,guard,nbytes,ecc", [(64, 2, False, 400, 0), (64, 6, True, 560, 0), (64, 1, True, 37, 0),
                                                    (64, 6, True, 320, 1), (1024, 6, True, 3000, 1),
                                                    (4096, 8, True, 6000, 0), (256, 4, False, 0, 0)])
def test_tx_encode_batch(api, orc, n, mod, guard, nbytes, ecc):
    import torch
    rng = np.random.default_rng(n + mod + nbytes)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc)
    nfr = 3
    pay = rng.integers(0, 256, (nfr, max(nbytes, 1)), dtype=np.uint8)[:, :nbytes]
    pay_t = torch.from_numpy(np.ascontiguousarray(pay)).to(ctx.device).reshape(nfr, nbytes)
    frames = host(ctx.encode_batch(pay_t))
    for f in range(nfr):
        body = orc.hamming74_encode(bytes(pay[f])) if ecc else bytes(pay[f])
        want = orc.encode(body, guard, mod, n)
        assert frames[f].size == want.size == ctx.frame_samples(nbytes)
        assert rel_err(frames[f], want) <= TOL, f"frame {f}"
        assert abs(max(frames[f].real.max(), frames[f].imag.max()) - 1.0) < 1e-6


@pytest.mark.parametrize("n,mod,guard,nbytes", [(64, 6, True, 2300), (64, 1, True, 400), (64, 2, False, 1000), (128, 6, True, 200), (128, 2, False, 3), (256, 4, True, 700), (512, 8, True, 2000),
                                                 (512, 1, False, 100), (1024, 6, False, 2500), (2048, 4, True, 4000), (4096, 8, True, 9000),
                                                 (4096, 2, False, 2500)])
def test_tx_encode_mid_frames(api, orc, n, mod, guard, nbytes):
    """k_txframe_mid / k_txframe4096 (encode in one HBM pass for N = 128 .. 4096 and for N = 64 frames of more than 56 data
    symbols: symbols stored divided by the header maximum while the frame maximum forms; test_tx_encode_frames_louder_than_their_header
    covers the rebuild) against the oracle's encode, 11 frames with ragged payload lengths on a 2-workgroup grid (several rounds per workgroup, a last
    round that is only partly filled).  src/transmitter.rs:11-58, 184-188."""
    import torch
    rng = np.random.default_rng(n + mod + nbytes)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 2})
    nfr = 11
    lens = rng.integers(0, nbytes + 1, nfr).astype(np.int32)
    lens[0], lens[-1] = nbytes, 0
    pay = rng.integers(0, 256, (nfr, nbytes), dtype=np.uint8)
    frames = host(ctx.encode_batch(torch.from_numpy(pay).to(ctx.device), lens=torch.from_numpy(lens)))
    S, D = n + n // 4, ctx.data_symbols(nbytes)
    # frames whose data symbols fit ONE workgroup step of the R x 64 kernel (D <= 32 / R) are built once, the others twice
    mid = "k_txframe_mid<once>" if n >= 512 and D <= 32 // (n // 64) else "k_txframe_mid"   # (N <= 256: the optimistic form at four waves per SIMD is faster)
    assert ctx.last_dispatch() == ("k_txframe4096" if n == 4096 else mid if n > 64 or D > 56 else "k_txframe64")
    assert frames.shape == (nfr, (10 + D) * S)
    for f in range(nfr):
        # up to its own last data symbol the frame equals the oracle's frame for that payload: the pilot-only symbols that
        # fill the slot are below the frame maximum, so the normalisation is the same (as test_tx_encode_ragged_lengths)
        want = orc.encode(bytes(pay[f, :lens[f]]), guard, mod, n)
        assert rel_err(frames[f, :want.size], want) <= TOL, f"frame {f} (len {lens[f]})"
        tail = frames[f, want.size:]
        assert tail.size % S == 0 and (tail.size == 0 or np.abs(tail).max() <= np.abs(frames[f, :want.size]).max())
        assert abs(max(frames[f].real.max(), frames[f].imag.max()) - 1.0) < 1e-6

@pytest.mark.parametrize("n,mod,nsym", [(64, 2, 60), (128, 2, 20), (256, 6, 16), (1024, 4, 5), (4096, 2, 3)])
def test_tx_encode_frames_louder_than_their_header(api, orc, n, mod, nsym):
    """The frame encoders store every data symbol divided by the HEADER maximum while the frame's own maximum forms, and build a round
    again only if a frame turned out louder than its header blocks (normalize, src/transmitter.rs:184-188 divides by the maximum of the
    whole frame).  Ordinary payloads never are (the header carries the full-scale locking signal); these are crafted to be, 2.5 x: loud
    and ordinary frames side by side in one workgroup round must equal the oracle and the build-twice scheme (tuning
    no_txframe_optimistic) bit for bit."""
    import torch
    nbytes = nsym * (n * mod // 8) - 16
    S = n + n // 4
    pays = [np.random.default_rng(5).integers(0, 256, nbytes, dtype=np.uint8), loud_payload(orc, n, mod, nbytes, 1, 1),
            np.random.default_rng(6).integers(0, 256, nbytes, dtype=np.uint8), loud_payload(orc, n, mod, nbytes, nsym - 1, 2),
            loud_payload(orc, n, mod, nbytes, 2, 3), np.random.default_rng(7).integers(0, 256, nbytes, dtype=np.uint8),
            np.zeros(nbytes, np.uint8)]
    pay = np.stack(pays)
    a = api.Context(n_fft=n, modulation=mod, guard_bands=False, tuning={"grid_cap": 2})
    b = api.Context(n_fft=n, modulation=mod, guard_bands=False, tuning={"grid_cap": 2, "no_txframe_optimistic": 1})
    fa = host(a.encode_batch(dev(a, pay)))
    fb = host(b.encode_batch(dev(b, pay)))
    assert a.last_dispatch() == b.last_dispatch() == ("k_txframe4096" if n == 4096 else "k_txframe_mid")
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    louder = 0
    for f in range(len(pays)):
        want = orc.encode(bytes(pay[f]), False, mod, n)
        assert rel_err(fa[f], want) <= TOL, f"frame {f}"
        louder += max(want[:10 * S].real.max(), want[:10 * S].imag.max()) < 0.5
    assert louder == 3


# ------------------------------------------------------------------ a10: decode (RX pipeline), config 3 shape
def run_decode_parity(api, orc, n, mod, guard, ecc, nbytes, nfr, span_extra, seed, snr_db=30.0, cfo_abs=False):
    import torch
    rng = np.random.default_rng(seed)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc,
                      cfo_mode=api.CFO_ABS if cfo_abs else api.CFO_SIGNED)
    flen = ctx.frame_samples(nbytes)
    D = ctx.data_symbols(nbytes)
    span = flen + span_extra
    caps, pays = [], []
    for f in range(nfr):
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        body = orc.hamming74_encode(pay) if ecc else pay
        tx = orc.encode(body, guard, mod, n)
        d = int(rng.integers(1, span_extra - 30))
        fd = (rng.random() * (0.95 if cfo_abs else 1.9) - (0.0 if cfo_abs else 0.95)) * np.pi / S
        caps.append(through_channel(orc, rng, tx, span, d, fd, snr_db, data_start=10 * S)); pays.append(pay)
    caps = np.stack(caps)
    res = ctx.decode_batch(dev(ctx, caps), max_symbols=D)
    ctx.synchronize()
    r = {k: host(v) for k, v in res.items()}
    nd = ctx.data_carriers
    n_excused = 0
    for f in range(nfr):
        w = orc.decode_sc(wide(caps[f]), guard, mod, n, window_reps=3, sync_lags=0, threshold=0.5, backoff=4,
                          cfo_abs=cfo_abs, max_symbols=D, want_soft=True)
        assert r["status"][f] == w["status"], f"frame {f}"
        if w["status"] != 0:
            assert r["len"][f] == 0
            continue
        assert r["offset"][f] == w["offset"] and abs(r["f_delta"][f] - w["f_delta"]) <= 1e-9
        got = bytes(r["bytes"][f][: r["len"][f]])
        want = orc.hamming74_decode(w["bytes"])[0] if ecc else w["bytes"]
        if got != want and not ecc:
            # excuse only decisions whose ORACLE soft value lies within TOL of a boundary.  Body bit b is stream bit
            # 128 + b (16-byte length header first), i.e. point (128 + b) // mod of the oracle's soft array.
            assert len(got) == len(want), f"frame {f}"
            gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
            wb = np.unpackbits(np.frombuffer(want, np.uint8), bitorder="little")
            pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
            from util import decision_margin
            margin = decision_margin(np.asarray(w["soft"])[pts], mod)
            assert np.all(margin < TOL), f"decode f={f}: {np.sum(margin >= TOL)} decisions differ away from any boundary"
            n_excused += int(pts.size)
        else:
            assert got == want, f"frame {f}"
    return n_excused, r, pays


def test_rx_decode_batch_config3(api, orc):
    n_excused, r, pays = run_decode_parity(api, orc, 64, 6, True, 0, 560, 40, 96, seed=31)
    assert n_excused <= 1
    ok = [f for f in range(40) if r["status"][f] == 0 and r["len"][f] == 560]
    assert len(ok) >= 36
    errs = sum(np.unpackbits(np.frombuffer(bytes(r["bytes"][f][:560]), np.uint8) ^ np.frombuffer(pays[f], np.uint8)).sum() for f in ok)
    assert errs / (len(ok) * 560 * 8) < 2e-3  # 64-QAM at 30 dB through the FIR channel


@pytest.mark.parametrize("n,mod,guard,ecc,nbytes,cfo_abs", [(64, 2, False, 0, 400, False), (64, 1, True, 0, 90, True),
                                                            (64, 6, True, 1, 320, False), (256, 4, True, 0, 700, False),
                                                            (1024, 6, True, 1, 3000, False)])
def test_rx_decode_batch_variants(api, orc, n, mod, guard, ecc, nbytes, cfo_abs):
    S = n + n // 4
    n_excused, r, pays = run_decode_parity(api, orc, n, mod, guard, ecc, nbytes, 6, S + 40, seed=n + mod + nbytes,
                                           snr_db=33.0, cfo_abs=cfo_abs)
    assert n_excused == 0
    good = [f for f in range(6) if r["status"][f] == 0]
    assert len(good) == 6
    errs = 0
    for f in good:  # loop-back BER: the FIR channel's weak bins (|H| ~ 0.3 near Nyquist) leave a few errors at 33 dB
        assert r["len"][f] >= len(pays[f])
        errs += orc.analysis(pays[f], bytes(r["bytes"][f][: len(pays[f])]))[0]
    assert errs / (6 * nbytes * 8) < 5e-3


@pytest.mark.parametrize("mod,guard,grid_cap", [(6, True, 0), (6, True, 3), (2, False, 2), (4, True, 0), (1, True, 0), (1, True, 2)])
def test_rxframe64_common_and_cut_bodies_as_two_launches(api, orc, mod, guard, grid_cap):
    """Round 4: k_rxframe64 runs as a pair -- the common frame body alone (four waves per SIMD with guard bands) over every frame,
    the capture-cut body over the device-side list of the frames the first launch had to leave.  Roomy captures (room for a whole
    frame + 64 samples) in which SOME frames start so late that the capture ends inside their data symbols, a noise-only slot and a
    slot too short to decode: status, offset, CFO, length and bytes must equal the oracle's and the one-kernel form's
    (tuning no_rxframe64_split), with the list walked by a capped grid as well."""
    rng = np.random.default_rng(64 + mod + grid_cap)
    nbytes = {6: 560, 2: 230, 4: 360, 1: 116 + 6 * grid_cap}[mod]   # BPSK with guard bands (6 bytes per symbol): 22 and 24 data symbols
    tune = {"grid_cap": grid_cap} if grid_cap else {}
    ctx = api.Context(n_fft=64, modulation=mod, guard_bands=guard, tuning=tune)
    one = api.Context(n_fft=64, modulation=mod, guard_bands=guard, tuning={**tune, "no_rxframe64_split": 1})
    flen, D = ctx.frame_samples(nbytes), ctx.data_symbols(nbytes)
    span = flen + 64 + 40
    nfr = 37
    delays = [int(rng.integers(1, 60)) if f % 3 else int(rng.integers(110, 700)) for f in range(nfr)]   # every third frame is cut
    caps = []
    for f in range(nfr):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, 64)
        caps.append(through_channel(orc, rng, tx, span, delays[f], (rng.random() * 1.8 - 0.9) * np.pi / 80, 30.0, data_start=800))
    caps[5] = fc32(0.003 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))                 # nothing to find
    caps = np.stack(caps)
    ra = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D).items()}
    assert ctx.last_dispatch().endswith("k_rxframe64<finish>+k_rxframe64<cut,list>"), ctx.last_dispatch()
    rb = {k: host(v) for k, v in one.decode_batch(dev(one, caps), max_symbols=D).items()}
    assert one.last_dispatch().endswith("k_rxframe64<finish>"), one.last_dispatch()
    n_cut = 0
    for f in range(nfr):
        w = orc.decode_sc(wide(caps[f]), guard, mod, 64, max_symbols=D)
        assert ra["status"][f] == rb["status"][f] == w["status"], f
        if w["status"] != 0:
            assert ra["len"][f] == rb["len"][f] == 0
            continue
        assert ra["offset"][f] == rb["offset"][f] == w["offset"] and abs(ra["f_delta"][f] - w["f_delta"]) <= 1e-9
        assert ra["len"][f] == rb["len"][f] == len(w["bytes"])
        got = bytes(ra["bytes"][f][: ra["len"][f]])
        assert got == bytes(rb["bytes"][f][: rb["len"][f]]), f       # the two forms agree bit for bit
        n_cut += (10 + D) * 80 > span - w["offset"]
        if got != w["bytes"]:                                          # a decision on the oracle's own boundary (never seen on these seeds)
            assert sum(a != b for a, b in zip(got, w["bytes"])) <= 1, f
    assert n_cut >= 8 and (ra["status"] == 0).sum() >= nfr - 3          # the cut body did run, on several frames


@pytest.mark.parametrize("ecc", [0, 1])
def test_rx_decode_reference_default_frames_take_the_frame_kernel(api, orc, ecc):
    """BPSK with guard bands -- the reference's own default, 6 bytes per symbol -- through k_rxframe64 (until round 5 its "whole dwords
    per symbol" gate sent exactly this shape to the generic kernels): ragged symbol counts, odd and even, so that a frame's last
    8-symbol group ends on half a dword, without and with the outer code (raw rows of an odd symbol count: stride rounded up to a dword)."""
    import torch
    rng = np.random.default_rng(600 + ecc)
    ctx = api.Context(n_fft=64, modulation=api.BPSK, guard_bands=True, ecc=api.ECC_HAMMING74 if ecc else api.ECC_NONE)
    maxb = 152 if ecc else 116                      # 47 / 22 data symbols per slot (the caller's rows of 116 bytes are dword-aligned: fused finish)
    lens = [maxb, 0, 4, 8, 12, 52, maxb - 4, 36, maxb] if ecc else [maxb, 0, 1, 5, 6, 7, 50, 107, 111, 33, 2, maxb]   # 107 bytes: 21 symbols, half a dword at the end
    D = ctx.data_symbols(maxb)
    assert D == (47 if ecc else 22)
    span = ctx.frame_samples(maxb) + 120
    caps, pays = [], []
    for ln in lens:
        pay = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        body = orc.hamming74_encode(pay) if ecc else pay
        tx = orc.encode(body, True, orc.BPSK, 64)
        caps.append(through_channel(orc, rng, tx, span, int(rng.integers(1, 70)), (rng.random() * 1.8 - 0.9) * np.pi / 80, 30.0))
        pays.append(pay)
    caps = np.stack(caps)
    r = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D).items()}
    want_d = "k_rxframe64+k_rxframe64<cut,list>+k_rx_finish" if ecc else "k_rxframe64<finish>+k_rxframe64<cut,list>"
    assert ctx.last_dispatch().endswith(want_d), ctx.last_dispatch()
    for f, ln in enumerate(lens):
        w = orc.decode_sc(wide(caps[f]), True, orc.BPSK, 64, max_symbols=D)
        want = orc.hamming74_decode(w["bytes"])[0] if ecc else w["bytes"]
        assert r["status"][f] == w["status"] == 0 and r["offset"][f] == w["offset"], f
        assert r["len"][f] == len(want), (f, ln, int(r["len"][f]), len(want))
        assert bytes(r["bytes"][f][: r["len"][f]]) == want, f
        assert bytes(r["bytes"][f][: ln]) == pays[f], f


@pytest.mark.parametrize("n,mod,guard", [(1024, 4, True), (1024, 6, False), (64, 6, True)])
def test_rx_decode_truncated_and_limited(api, orc, n, mod, guard):
    """The fused per-frame kernels (k_rxframe64 / k_rxframe1024) on captures that END inside a data symbol (pad_chunk,
    receiver.rs:203-210: the tail is zero-filled and demodulated as garbage, then cut by the length header) and with
    max_symbols smaller than the frame (fewer live symbols): status, offset and bytes equal the oracle's."""
    rng = np.random.default_rng(n + mod)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    nbytes = 900 if n == 1024 else 300
    D = ctx.data_symbols(nbytes)
    caps, cuts = [], []
    for f in range(6):
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        tx = orc.encode(pay, guard, mod, n)
        full = through_channel(orc, rng, tx, tx.size + 200, 20 + 7 * f, 0.002 * (f - 2) / (n / 64), 32.0, data_start=10 * S)
        cut = full.size if f == 0 else full.size - 200 - int(rng.integers(1, 2 * S))   # frames 1..5 lose part of their tail
        c = full.copy(); c[cut:] = 0
        caps.append(c); cuts.append(cut)
    caps = np.stack(caps)
    for max_sym in (D, max(1, D - 2)):
        res = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=max_sym).items()}
        for f in range(6):
            w = orc.decode_sc(wide(caps[f]), guard, mod, n, max_symbols=max_sym)
            assert res["status"][f] == w["status"], (f, max_sym)
            if w["status"] == 0:
                assert res["offset"][f] == w["offset"] and abs(res["f_delta"][f] - w["f_delta"]) <= 1e-9
                assert bytes(res["bytes"][f][: res["len"][f]]) == w["bytes"], (f, max_sym)


@pytest.mark.parametrize("mod,guard,ecc,cfo_mode", [(6, True, 0, 1), (6, True, 1, 1), (2, False, 0, 2), (4, True, 0, 0),
                                                     (8, False, 1, 1), (1, False, 0, 1), (8, True, 0, 2)])
def test_rx_decode_chain_with_both_detectors_and_oracle(api, orc, mod, guard, ecc, cfo_mode):
    """The N = 64 receive chain (k_sc80 / k_sc_cf + k_sc_post + k_rx_prepare + k_rxframe64 [+ k_rx_finish]) with either timing detector
    -- every output identical except the CFO (sums that differ in their last bits: <= 1e-13) and decisions the CFO's last bits can
    move -- and against the oracle, on a batch that mixes clean frames, noise-only slots (NOSYNC), captures cut inside the header
    (SHORT) or inside a data symbol (pad_chunk), and a limited symbol count.  src/receiver.rs:9-96.  (Rounds 2-4 ran a one-pass
    receive kernel through this test; it never beat the staged chain and was removed in round 5.)"""
    rng = np.random.default_rng(900 + mod + ecc + cfo_mode)
    ctx = api.Context(n_fft=64, modulation=mod, guard_bands=guard, ecc=ecc, cfo_mode=cfo_mode, rx_path=api.RX_STAGED)
    ctx1 = api.Context(n_fft=64, modulation=mod, guard_bands=guard, ecc=ecc, cfo_mode=cfo_mode, tuning={"no_sc80": 1})
    nbytes = 200 if mod > 1 else 100
    D = ctx.data_symbols(nbytes)
    flen = ctx.frame_samples(nbytes)
    span = (flen + 120) // 2 * 2
    assert span <= 2560
    caps, kinds = [], []
    for f in range(48):
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        body = orc.hamming74_encode(pay) if ecc else pay
        tx = orc.encode(body, guard, mod, 64)
        kind = ("ok", "ok", "ok", "noise", "cut_data", "cut_head")[f % 6]
        fd = (rng.random() * 1.9 - 0.95) * np.pi / 80 * (0.5 if cfo_mode == 2 else 1.0)
        if cfo_mode == 2:
            fd = abs(fd)
        c = through_channel(orc, rng, tx, span, int(rng.integers(1, 100)), fd, 30.0, data_start=800)
        if kind == "noise":
            c = fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))
        caps.append(c); kinds.append(kind)
    caps = np.stack(caps)
    frame_lens = {"full": span, "cut_data": flen - 100, "cut_head": 700}
    for label, flen_used in frame_lens.items():
        for max_sym in (D, max(1, D - 3)):
            one = {k: host(v) for k, v in ctx1.decode_batch(dev(ctx1, caps), max_symbols=max_sym, frame_len=flen_used).items()}
            assert ctx1.last_dispatch().startswith("k_sc_cf<") and "+k_rx_prepare+k_rxframe64" in ctx1.last_dispatch(), ctx1.last_dispatch()
            two = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=max_sym, frame_len=flen_used).items()}
            d2 = ctx.last_dispatch()
            assert d2.startswith("k_sc80+") and "<rx>" not in d2 and "+k_rx_prepare+k_rxframe64" in d2, d2
            assert np.array_equal(one["status"], two["status"]) and np.array_equal(one["offset"], two["offset"])
            assert np.array_equal(one["len"], two["len"])
            assert np.allclose(one["f_delta"], two["f_delta"], rtol=0, atol=1e-13)
            assert np.allclose(one["metric"], two["metric"], rtol=1e-6, atol=0)
            for f in range(caps.shape[0]):
                x = wide(caps[f][:flen_used])
                w = orc.decode_sc(x, guard, mod, 64, window_reps=3, sync_lags=0, threshold=0.5, backoff=4,
                                  cfo_abs=cfo_mode == 2, cfo_off=cfo_mode == 0, max_symbols=max_sym, want_soft=True)
                assert one["status"][f] == w["status"], (label, max_sym, f, kinds[f])
                if w["status"] != 0:
                    assert one["len"][f] == 0
                    continue
                assert one["offset"][f] == w["offset"] and abs(one["f_delta"][f] - w["f_delta"]) <= 1e-12
                got = bytes(one["bytes"][f][: one["len"][f]])
                want = orc.hamming74_decode(w["bytes"])[0] if ecc else w["bytes"]
                if got != want:   # only a decision the oracle itself has within TOL of a boundary may differ
                    assert not ecc and len(got) == len(want), (label, max_sym, f)
                    gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
                    wb = np.unpackbits(np.frombuffer(want, np.uint8), bitorder="little")
                    pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
                    from util import decision_margin
                    assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), (label, max_sym, f)
        if label == "full":
            assert int((one["status"] == 0).sum()) >= 36 and int((one["status"] == -2).sum()) >= 6


# ------------------------------------------------------------------ EXT-3 for long periods (kernels_scbig.hip), EXT-4 decode up to N = 4096
def test_long_period_fine_tiles_agree(api):
    """k_scb_fine<5> (320-lag tiles, the default for N <= 2048) and k_scb_fine<10> (640-lag tiles, tuning "scb_big_tiles") walk the
    same exact sums in different tile sizes: identical timing index, CFO to 1e-12 and metric to 1e-6 on 96 N = 1024 captures from the library's
    TX and GPU channel (each tiling is compared with the oracle in test_sc_correlate_and_decode_long_periods)."""
    import math
    import torch
    ctx = api.Context(n_fft=1024, modulation=api.QAM16, guard_bands=True)
    g = torch.Generator(device=ctx.device); g.manual_seed(5)
    nfr = 96
    pay = torch.randint(0, 256, (nfr, 700), dtype=torch.uint8, device=ctx.device, generator=g)
    tx = ctx.encode_batch(pay)
    d = torch.randint(1, 1281, (nfr,), device=ctx.device, generator=g, dtype=torch.int32)
    fd = (torch.rand((nfr,), device=ctx.device, generator=g, dtype=torch.float64) * 1.8 - 0.9) * math.pi / ctx.S
    x = ctx.channel_batch(tx, snr_db=35.0, seed=9, delay=d, f_delta=fd, span=tx.shape[1] + 1536)
    ctx.set_tuning("no_sc_stream", 1)            # N = 1024 is served by the streaming detector by default: this test is about the two-pass kernels
    small = [host(v) for v in ctx.sc_correlate(x)]
    assert ctx.last_dispatch() == "k_scb_chunks<contig>+k_scb_fine<5>"
    ctx.set_tuning("scb_big_tiles", 1)
    big = [host(v) for v in ctx.sc_correlate(x)]
    assert ctx.last_dispatch() == "k_scb_chunks<contig>+k_scb_fine<10>"
    assert (small[0] >= 0).all() and np.array_equal(small[0], big[0])
    # the f64 sums are accumulated in a different order: equal to rounding, not to the bit
    assert np.abs(small[1] - big[1]).max() <= 1e-12 and np.abs(small[2] - big[2]).max() <= 1e-6


@pytest.mark.parametrize("reps", [3, 1, 2])
@pytest.mark.parametrize("n", [128, 256, 512, 1024, 2048, 4096])
def test_sc_stream_detector_against_the_oracle(api, orc, n, reps):
    """k_sc_stream (kernels_scstream.hip): the one-pass, early-exit Schmidl-Cox detector for L = 160 .. 1280, against the oracle's
    exhaustive search (orc_sc_sync) -- timing index bit-exact, CFO to 1e-9, metric to 1e-6 -- on a 2-wavefront grid (many frames per
    wavefront, the DMA ring restarted per frame), with: packets at delays from 1 sample to most of a period (first crossing in the
    first tiles and late), noise-only captures (the whole capture is streamed, no crossing), a packet so late that the capture
    ends inside its peak window, captures cut inside the preamble, a strong and a weak packet in one capture (the FIRST crossing
    wins), searches bounded to a few tiles, odd capture lengths (odd row strides), and window lengths W = L, 2 L, 3 L; the same rows
    from an 8-byte aligned base, and through the two-pass kernels (lab key no_sc_stream).  (North-star extension: parity pinned by the
    build's oracle only)"""
    import torch
    rng = np.random.default_rng(4242 + n + reps)
    S = n + n // 4
    W = reps * S
    ctx = api.Context(n_fft=n, modulation=api.QAM16, guard_bands=True, sync_window_reps=reps, tuning={"grid_cap": 2})
    nbytes = 40 * (n // 64)
    txs = [orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), True, 4, n) for _ in range(3)]
    flen = txs[0].size
    span = (flen + 2 * S + 37) // 2 * 2 + (1 if n == 256 else 0)          # one length is odd (ragged last 16-byte piece)
    caps = []
    for f, delay in enumerate([1, 7, S // 3, S - 3, S + 11, 2 * S - 40]):
        caps.append(through_channel(orc, rng, txs[f % 3], span, delay, (rng.random() * 1.6 - 0.8) * np.pi / S, 30.0, data_start=10 * S))
    caps.append(fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))))                 # noise only
    late = np.zeros(span, np.complex128)
    late[span - 6 * S:] = txs[0][: 6 * S]                                                                   # the capture ends inside the window
    caps.append(fc32(late + 0.003 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))))
    cut = caps[2].copy(); cut[int(3.4 * S):] = 0                                                           # ends inside the preamble
    caps.append(cut)
    two = 0.3 * wide(caps[1]) + np.roll(wide(caps[3]), 3 * S)                                              # weak early packet, strong late one
    caps.append(fc32(two))
    caps.append(np.zeros(span, np.complex64))                                                              # all zeros: no metric defined anywhere
    caps = np.stack(caps)
    xd = dev(ctx, caps)
    aligned = True                            # (round 5: LDS-DMA takes rows of any alignment and odd strides, test_streaming_detectors_on_rows_of_any_alignment)
    for lags in (0, 700, 2 * S + 5, 64):
        d_hat, f_delta, metric = (host(v) for v in ctx.sc_correlate(xd, n_lags=lags))
        disp = ctx.last_dispatch()
        # short windows that fit one LDS tile (W + 20 <= 320: N = 128 with W = L) belong to the one-tile kernel k_sc_cf
        fast = disp.startswith("k_sc_cf<")
        assert fast or disp.startswith("k_sc_stream") == aligned, (disp, span)
        assert not fast or W + 20 <= 320, (disp, W)
        # a period of one or two 640-sample tiles (N = 512, 1024) keeps the partner micro-chunk in the producer's registers: another instantiation
        assert fast or disp == ("k_sc_stream<regs>" if n in (512, 1024) else "k_sc_stream"), (disp, n)
        for f in range(caps.shape[0]):
            wd, wp, wm, wfd = orc.sc_sync(wide(caps[f]), L=S, window_reps=reps, n_lags=lags, threshold=0.5)
            assert d_hat[f] == wd, (n, reps, lags, f, int(d_hat[f]), wd)
            if wd >= 0:
                assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6 * max(1.0, wm), (n, reps, lags, f)
    # the same captures one sample into a buffer (8-byte aligned rows) through the same kernel, and through the two-pass kernels (lab key)
    buf = torch.zeros(caps.size + 2, dtype=torch.complex64, device=ctx.device)
    sh = buf[1:1 + caps.size].view(caps.shape)
    sh.copy_(xd)
    d2 = host(ctx.sc_correlate(sh)[0])
    assert ctx.last_dispatch().startswith("k_sc_stream") or W + 20 <= 320, ctx.last_dispatch()
    assert np.array_equal(d2, host(ctx.sc_correlate(xd)[0]))
    two = api.Context(n_fft=n, modulation=api.QAM16, guard_bands=True, sync_window_reps=reps, tuning={"no_sc_stream": 1})
    d3 = host(two.sc_correlate(dev(two, caps))[0])
    assert "k_sc_stream" not in two.last_dispatch()
    assert np.array_equal(d2, d3)


@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("n,mod,nbytes", [(128, 4, 300), (256, 6, 700), (512, 2, 500), (1024, 6, 1304), (2048, 4, 3000), (4096, 8, 9000)])
def test_sc_correlate_and_decode_long_periods(api, orc, n, mod, nbytes, two_pass):
    """Schmidl-Cox for L = 160 .. 5120 -- the streaming detector k_sc_stream, and (two_pass: tuning no_sc_stream) the chunk sums +
    bounded exact search of kernels_scbig.hip -- against the oracle over ALL lags of the capture
    and over a bounded search, on frames through the FIR channel with delay, CFO and noise, on noise-only captures and on a
    capture cut inside the preamble; then the whole decode (N = 2048 / 4096 included: ADVICE r1).  Timing index, status and
    offset bit-exact, CFO to 1e-9, bytes exact."""
    rng = np.random.default_rng(7000 + n)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True, tuning={"no_sc_stream": int(two_pass)})
    D = ctx.data_symbols(nbytes)
    flen = ctx.frame_samples(nbytes)
    span = (flen + 3 * S // 2) // 2 * 2
    nf = 5 if n <= 1024 else 3
    caps = long_period_captures(orc, rng, n, mod, nbytes, nf, span)
    for lags in (0, 2 * S):
        xd = dev(ctx, caps)
        d_hat, f_delta, metric = (host(v) for v in ctx.sc_correlate(xd, n_lags=lags))
        if xd.data_ptr() % 16 == 0:
            assert ("k_sc_stream" in ctx.last_dispatch()) == (not two_pass), ctx.last_dispatch()
        for f in range(caps.shape[0]):
            wd, wp, wm, wfd = orc.sc_sync(wide(caps[f]), L=S, window_reps=3, n_lags=lags, threshold=0.5)
            assert d_hat[f] == wd, (n, lags, f, d_hat[f], wd)
            if wd >= 0:
                assert abs(f_delta[f] - wfd) <= 1e-9 and abs(metric[f] - wm) <= 1e-6 * max(1.0, wm)
    res = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D).items()}
    for f in range(caps.shape[0]):
        w = orc.decode_sc(wide(caps[f]), True, mod, n, max_symbols=D, want_soft=True)
        assert res["status"][f] == w["status"], (n, f)
        if w["status"] != 0:
            continue
        assert res["offset"][f] == w["offset"] and abs(res["f_delta"][f] - w["f_delta"]) <= 1e-9
        got = bytes(res["bytes"][f][: res["len"][f]])
        if got != w["bytes"]:
            assert len(got) == len(w["bytes"])
            gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
            wb = np.unpackbits(np.frombuffer(w["bytes"], np.uint8), bitorder="little")
            pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
            from util import decision_margin
            assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), (n, f)
    assert int((res["status"][:nf] == 0).sum()) == nf


def test_bounded_search_clips_the_peak_window(api, orc):
    """n_lags bounds the searched lags AND therefore the peak window [d1, min(d1 + W, n_lags - 1)] (include/ofdm_hip.h):
    a frame whose true peak lies beyond n_lags - 1 gets a different (earlier) timing from a bounded search than from the
    full one -- on the GPU exactly as in the oracle.  (This is why 8 of 262 144 round-1 config-3 frames decoded differently
    with n_lags = 256: their first crossing came late enough for the clipped window to miss the peak.)"""
    rng = np.random.default_rng(88)
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64, 64)
    cap = through_channel(orc, rng, tx, 2400, 150, 0.01, 30.0, data_start=800)   # peak at 150 + 89 = 239
    x = dev(ctx, cap.reshape(1, -1))
    full = int(host(ctx.sc_correlate(x)[0])[0])
    assert full == orc.sc_sync(wide(cap), 80, 3, 0, 0.5)[0] == 239
    for lags in (200, 230, 239, 240, 256):
        got = int(host(ctx.sc_correlate(x, n_lags=lags)[0])[0])
        want = orc.sc_sync(wide(cap), 80, 3, lags, 0.5)[0]
        assert got == want, (lags, got, want)
        assert (got == full) == (lags >= 240)        # the window is clipped at lag n_lags - 1
    # and the decode follows: status / offset / bytes equal the oracle's under the bounded search too
    res = {k: host(v) for k, v in ctx.decode_batch(x, max_symbols=16, n_lags=230).items()}
    w = orc.decode_sc(wide(cap), True, orc.QAM64, 64, sync_lags=230, max_symbols=16)
    assert res["status"][0] == w["status"] and res["offset"][0] == w["offset"]


# ------------------------------------------------------------------ a11 / a12: the reference's own timing (xcorr_fft, offset = lag - 1)
def test_xcorr_reference_kats_and_oracle(api, orc):
    """ofdm_xcorr_batch = SignalRef::xcorr_fft (src/signals/mod.rs:186-217) on the GPU: the reference's two known answers
    (signals/mod.rs:420-441: [1,2,3] x [4,5] -> [0,5,14,23,12], idx_max 3; the 8 / 4 sample pair -> idx_max 7), and
    against the oracle's FFT-based restatement on a capture with the locking signal (the decode use): idx_max exact,
    outputs <= 1e-5."""
    import json, os
    ctx = api.Context()
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))["xcorr"]
    for case in kat:
        a = np.asarray(case["a"], np.complex64); b = np.asarray(case["b"], np.complex64)
        idx, pk, out = ctx.xcorr(dev(ctx, a.reshape(1, -1)), dev(ctx, b), want_out=True)
        assert int(host(idx)[0]) == case["idx_max"]
        np.testing.assert_allclose(host(out)[0].real, case["full"], atol=1e-5)
    a = np.array([1, 2, 3], np.complex64); b = np.array([4, 5], np.complex64)
    idx, pk, out = ctx.xcorr(dev(ctx, a.reshape(1, -1)), dev(ctx, b), want_out=True)
    np.testing.assert_allclose(host(out)[0], [0, 5, 14, 23, 12], atol=1e-6)
    assert int(host(idx)[0]) == 3 and abs(float(host(pk)[0]) - 23.0) < 1e-5
    a = np.array([1, 1, 0, 0, 1, 1, 0, 0], np.complex64); b = np.array([1, 1, 0, 0], np.complex64)
    idx, pk, out = ctx.xcorr(dev(ctx, a.reshape(1, -1)), dev(ctx, b), want_out=True)
    np.testing.assert_allclose(host(out)[0], [0, 0, 0, 0, 0, 0, 1, 2, 1, 0, 1, 2, 1, 0, 0], atol=1e-6)
    assert int(host(idx)[0]) == 7
    # against the oracle on captures (complex b, several tiles of lags, a batch)
    rng = np.random.default_rng(11)
    lock = fc32(orc.locking_signal(80))
    caps = []
    for f in range(4):
        tx = orc.encode(bytes(rng.integers(0, 256, 600, dtype=np.uint8)), True, orc.QAM64)
        caps.append(through_channel(orc, rng, tx, 5000, int(rng.integers(1, 300)), 0.003 * f, 25.0, data_start=800))
    caps = np.stack(caps)
    idx, pk, out = ctx.xcorr(dev(ctx, caps), dev(ctx, lock), want_out=True)
    bz = fc32(rng.standard_normal(37) + 1j * rng.standard_normal(37))
    idx2, pk2, out2 = ctx.xcorr(dev(ctx, caps), dev(ctx, bz), want_out=True)
    for f in range(4):
        wi, wout = orc.xcorr_fft(wide(caps[f]), wide(lock))
        assert int(host(idx)[f]) == wi and rel_err(host(out)[f], wout) <= TOL
        assert abs(float(host(pk)[f]) - abs(wout[wi])) <= 1e-5 * abs(wout[wi])
        wi, wout = orc.xcorr_fft(wide(caps[f]), wide(bz))
        assert int(host(idx2)[f]) == wi and rel_err(host(out2)[f], wout) <= TOL
    z = ctx.xcorr(dev(ctx, np.zeros((1, 100), np.complex64)), dev(ctx, lock))
    assert int(host(z[0])[0]) == 0 and float(host(z[1])[0]) == 0.0      # nothing exceeds the start value 0: idx_max stays 0


@pytest.mark.parametrize("n,mod,guard,nbytes", [(64, 2, False, 400), (64, 6, True, 560), (1024, 4, True, 1500)])
def test_rx_decode_reference_sync_mode(api, orc, n, mod, guard, nbytes):
    """decode with the reference's own detector pair (OFDM_SYNC_REFERENCE: xcorr_fft timing, offset = lag - 1, quirk Q1;
    frequency_correction CFO with its abs(), quirk Q2) against the oracle's decode_ref (src/receiver.rs:9-96 as written):
    status, offset, CFO (1e-9) and bytes, including the zero-delay capture the reference panics on (offset -1)."""
    rng = np.random.default_rng(12 + n + mod)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, sync_mode=api.SYNC_REFERENCE, cfo_mode=api.CFO_ABS)
    D = ctx.data_symbols(nbytes)
    flen = ctx.frame_samples(nbytes)
    span = flen + 2 * S
    caps = []
    for f in range(6):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, n)
        d = int(rng.integers(2, S))
        fd = rng.random() * 0.5 * np.pi / S
        caps.append(through_channel(orc, rng, tx, span, d, fd, 33.0, data_start=10 * S))
    tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, n)
    z = np.zeros(span, np.complex64); z[: tx.size] = fc32(tx)          # zero delay, no channel: lag 0 -> offset -1
    caps.append(z)
    caps.append(caps[0][: span].copy()); caps[-1][9 * S:] = 0            # too short after trimming
    caps = np.stack(caps)
    res = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D + 2).items()}
    n_ok = 0
    for f in range(caps.shape[0]):
        w = orc.decode_ref(wide(caps[f]), guard, mod, n, want_soft=True)
        assert res["status"][f] == w["status"], (f, res["status"][f], w["status"])
        assert res["offset"][f] == w["offset"], f
        if w["status"] != 0:
            assert res["len"][f] == 0
            continue
        n_ok += 1
        assert abs(res["f_delta"][f] - w["f_delta"]) <= 1e-9
        got = bytes(res["bytes"][f][: res["len"][f]])
        if got != w["bytes"]:
            assert len(got) == len(w["bytes"])
            gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
            wb = np.unpackbits(np.frombuffer(w["bytes"], np.uint8), bitorder="little")
            pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
            from util import decision_margin
            assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), f
    assert n_ok >= 5 and res["status"][6] == -3 and res["offset"][6] == -1


@pytest.mark.parametrize("n,mod,guard,nbytes", [(256, 4, True, 300), (4096, 6, True, 5000)])
def test_rx_decode_reference_mode_negative_offsets_first(api, orc, n, mod, guard, nbytes):
    """OFDM_SYNC_REFERENCE reports offset = idx_max - N (src/receiver.rs:21): -N for an all-zero capture (idx_max stays 0,
    src/signals/mod.rs:206-207) and -1 for a zero-delay one (quirk Q1).  For the lengths whose chain is the generic channel
    estimate + k_demod_mid / k_demod4096 (N outside {64, 1024}) that value used to reach fetches that only test an upper
    bound.  Here those two captures come FIRST (a read in front of row 0 is a read in front of the allocation), on a
    2-workgroup grid so that their dead symbols are followed by live ones in the same workgroup slot."""
    rng = np.random.default_rng(21 + n + mod)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, sync_mode=api.SYNC_REFERENCE, cfo_mode=api.CFO_ABS,
                      tuning={"grid_cap": 2})
    D = ctx.data_symbols(nbytes)
    flen = ctx.frame_samples(nbytes)
    span = flen + S
    caps = [np.zeros(span, np.complex64)]                                # all-zero: idx_max 0 -> offset -span
    tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, n)
    z = np.zeros(span, np.complex64); z[: tx.size] = fc32(tx)            # zero delay, no channel: lag 0 -> offset -1
    caps.append(z)
    for f in range(4):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), guard, mod, n)
        caps.append(through_channel(orc, rng, tx, span, int(rng.integers(2, S // 2)), rng.random() * 0.5 * np.pi / S, 34.0,
                                    data_start=10 * S))
    caps = np.stack(caps)
    res = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=D + 2).items()}
    disp = ctx.last_dispatch()
    assert disp == "k_xcorr+k_rx_prepare_ref+k_freq_corr+k_sym<chest>+" + ("k_demod4096<frame>" if n == 4096 else "k_demod_mid<frame>") + "+k_rx_finish", disp
    assert list(res["status"][:2]) == [-3, -3] and list(res["offset"][:2]) == [-span, -1] and list(res["len"][:2]) == [0, 0]
    for f in range(caps.shape[0]):
        w = orc.decode_ref(wide(caps[f]), guard, mod, n, want_soft=True)
        assert res["status"][f] == w["status"] and res["offset"][f] == w["offset"], (f, res["status"][f], w["status"])
        if w["status"] != 0:
            continue
        assert abs(res["f_delta"][f] - w["f_delta"]) <= 1e-9
        got = bytes(res["bytes"][f][: res["len"][f]])
        if got != w["bytes"]:
            assert len(got) == len(w["bytes"])
            gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
            wb = np.unpackbits(np.frombuffer(w["bytes"], np.uint8), bitorder="little")
            pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
            from util import decision_margin
            assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), f
    assert int((res["status"][2:] == 0).sum()) == 4


@pytest.mark.parametrize("grid_cap", [1, 2, 3])
@pytest.mark.parametrize("n,mod,nbytes", [(512, 2, 700), (4096, 6, 5000), (128, 4, 200), (2048, 8, 6000)])
def test_rx_decode_dead_symbols_precede_live_ones(api, orc, n, mod, nbytes, grid_cap):
    """A dead symbol -- one past a frame's live count (failed sync, short capture, max_symbols above the frame's own count) --
    must leave the demodulator's packed LDS image untouched: nothing flushes or clears it after such a step, and demap(0)
    is non-zero for every modulation above BPSK, so stale bits would be OR-ed into the next LIVE symbol of the same
    (workgroup, slot) of the persistent loop (k_demod_mid<FRAME> / k_demod4096<FRAME>).  The no-sync and the short
    frame come FIRST, max_symbols exceeds every frame's own count, and the grid is capped at 1 .. 3 workgroups so that the
    dead steps are followed by live ones in the same slot.  Bytes, lengths, status against orc.decode_sc.  src/receiver.rs:64-95."""
    rng = np.random.default_rng(555 + n + mod)
    S = n + n // 4
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=True, tuning={"grid_cap": grid_cap})
    D = ctx.data_symbols(nbytes)
    flen = ctx.frame_samples(nbytes)
    span = (flen + S // 2 + 80) // 2 * 2            # room for the delay, less than one more whole symbol
    max_sym = D + 3
    caps = [fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))]          # noise only: NOSYNC, 0 live symbols
    for f in range(6):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), True, mod, n)
        c = through_channel(orc, rng, tx, span, int(rng.integers(1, 60)), (rng.random() * 1.6 - 0.8) * np.pi / S, 34.0, data_start=10 * S)
        if f == 0:
            c[flen - 2 * S:] = 0                      # ends two symbols early: fewer live symbols than the others
        if f == 3:
            c = fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))      # a dead frame in the middle too
        caps.append(c)
    caps = np.stack(caps)
    res = {k: host(v) for k, v in ctx.decode_batch(dev(ctx, caps), max_symbols=max_sym).items()}
    assert ("k_demod4096<frame>" if n == 4096 else "k_demod_mid<frame>") in ctx.last_dispatch(), ctx.last_dispatch()
    n_ok = 0
    for f in range(caps.shape[0]):
        w = orc.decode_sc(wide(caps[f]), True, mod, n, max_symbols=max_sym, want_soft=True)
        assert res["status"][f] == w["status"], (f, res["status"][f], w["status"])
        if w["status"] != 0:
            assert res["len"][f] == 0
            continue
        n_ok += 1
        assert res["offset"][f] == w["offset"]
        got = bytes(res["bytes"][f][: res["len"][f]])
        if got != w["bytes"]:
            assert len(got) == len(w["bytes"]), (f, len(got), len(w["bytes"]))
            gb = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
            wb = np.unpackbits(np.frombuffer(w["bytes"], np.uint8), bitorder="little")
            pts = np.unique((128 + np.nonzero(gb != wb)[0]) // mod)
            from util import decision_margin
            assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), (f, pts[:8])
    assert res["status"][0] == -2 and res["status"][4] == -2 and n_ok >= 4


@pytest.mark.parametrize("ecc", [0, 1])
@pytest.mark.parametrize("mod,guard", [(6, True), (4, False)])
def test_rxframe1024_ring_across_frames_and_finish_modes(api, orc, mod, guard, ecc):
    """k_rxframe1024 (kernels_rx1024.hip): the LDS-DMA sample ring runs ACROSS frames, so a 1- and a 2-workgroup grid make every
    workgroup stream many frames back to back -- with dead frames (noise only: no sync) first, in the middle and last, a
    capture cut inside a data symbol (that item takes the synchronous zero-filling path, pad_chunk receiver.rs:203-210), odd
    and even start offsets (the one-sample shift of the aligned DMA image), and more symbols asked for than some frames hold.
    Three ways through the kernel must give the oracle's bytes: the fused finish (header, truncate, Hamming decode from the LDS
    image), raw bytes + k_rx_finish (tuning no_rx1024_finish), and an 8-byte-aligned batch (no LDS-DMA at all).
    src/receiver.rs:44-95, 212-229."""
    import torch
    rng = np.random.default_rng(1024 + mod + ecc)
    n, S = 1024, 1280
    ctx0 = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc)
    nbytes = 1000
    D = ctx0.data_symbols(nbytes)
    flen = ctx0.frame_samples(nbytes)
    span = (flen + S // 2 + 64) // 2 * 2
    caps, offs = [], []
    for f in range(11):
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        body = orc.hamming74_encode(pay) if ecc else pay
        tx = orc.encode(body, guard, mod, n)
        c = through_channel(orc, rng, tx, span, 3 + 5 * f, (rng.random() * 1.6 - 0.8) * np.pi / S, 35.0, data_start=10 * S)
        if f in (0, 5, 10):
            c = fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span)))     # dead frames
        if f == 7:
            c[flen - S - 200:] = 0                                                            # ends inside the last-but-one data symbol
        caps.append(c)
    caps = np.stack(caps)
    want = [orc.decode_sc(wide(caps[f]), guard, mod, n, max_symbols=D + 1, want_soft=True) for f in range(caps.shape[0])]
    assert {w["offset"] & 1 for w in want if w["status"] == 0} == {0, 1}                       # both parities of the DMA shift
    buf = torch.zeros(caps.size + 2, dtype=torch.complex64, device=ctx0.device)
    shifted = buf[1:1 + caps.size].view(caps.shape)                                           # 8-byte aligned rows
    shifted.copy_(torch.from_numpy(caps).to(ctx0.device))
    assert shifted.data_ptr() % 16 == 8
    for grid_cap in (1, 2):
        for mode in ("fused", "unfused", "unaligned"):
            tuning = {"grid_cap": grid_cap}
            if mode == "unfused":
                tuning["no_rx1024_finish"] = 1
            ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=ecc, tuning=tuning)
            x = shifted if mode == "unaligned" else dev(ctx, caps)
            res = {k: host(v) for k, v in ctx.decode_batch(x, max_symbols=D + 1).items()}
            disp = ctx.last_dispatch()
            assert ("k_rxframe1024<finish>" in disp) == (mode != "unfused") and ("k_rx_finish" in disp) == (mode == "unfused"), disp
            for f, w in enumerate(want):
                assert res["status"][f] == w["status"], (mode, grid_cap, f)
                if w["status"] != 0:
                    assert res["len"][f] == 0, (mode, grid_cap, f)
                    continue
                assert res["offset"][f] == w["offset"]
                got = bytes(res["bytes"][f][: res["len"][f]])
                wb = orc.hamming74_decode(w["bytes"])[0] if ecc else w["bytes"]
                if got != wb:
                    assert not ecc and len(got) == len(wb), (mode, grid_cap, f, len(got), len(wb))
                    g1 = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
                    w1 = np.unpackbits(np.frombuffer(wb, np.uint8), bitorder="little")
                    pts = np.unique((128 + np.nonzero(g1 != w1)[0]) // mod)
                    from util import decision_margin
                    assert np.all(decision_margin(np.asarray(w["soft"])[pts], mod) < TOL), (mode, grid_cap, f)
            assert int((res["status"] == 0).sum()) == 8 and list(res["status"][[0, 5, 10]]) == [-2, -2, -2]


def _misaligned_u8(ctx, n, nb):
    import torch
    buf = torch.zeros(n * nb + 8, dtype=torch.uint8, device=ctx.device)
    out = buf[1:1 + n * nb].view(n, nb)
    assert out.data_ptr() % 4 == 1 and out.is_contiguous()
    return out


def _misaligned_c64(ctx, rows, cols):
    import torch
    buf = torch.zeros(rows * cols + 4, dtype=torch.complex64, device=ctx.device)
    out = buf[1:1 + rows * cols].view(rows, cols)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    return out


@pytest.mark.parametrize("n,mod", [(64, 6), (512, 4), (4096, 8)])
def test_misaligned_outputs_take_the_generic_kernels_and_still_match(api, orc, n, mod):
    """Every shape-specialised launcher declines requests outside its envelope (hipErrorNotSupported) and the C ABI falls
    back to the generic k_sym.  One deliberately misaligned output per launcher -- a byte-misaligned row base for the RX
    demodulators (k_demod64 / k_demod_mid / k_demod4096), an 8-byte-aligned sample buffer for the TX stream kernels
    (k_tx_mid / k_tx4096) and the one-pass encoders (k_txframe64 / k_txframe_mid / k_txframe4096) -- must (a) be reported
    as served by the generic kernel and (b) still equal the oracle.  The aligned twin of each call must report the
    specialised kernel: removing a run_* call from ofdm_abi.hip turns this red.  src/receiver.rs:99-190, src/transmitter.rs:11-58."""
    import torch
    rng = np.random.default_rng(n + mod)
    guard = True
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    S, k, nf = n + n // 4, 8, 5
    fast_rx = {64: "k_demod64", 512: "k_demod_mid", 4096: "k_demod4096"}[n]
    fast_tx = "k_tx4096" if n == 4096 else "k_tx_mid"
    fast_enc = {64: "k_txframe64", 512: "k_txframe_mid", 4096: "k_txframe4096"}[n]
    # ---- RX demod
    x, data = make_symbols_np(orc, rng, k * nf, n, guard, mod, snr_db=38.0)
    want, wsoft = orc.rx_demod(wide(x), n, guard, mod, want_soft=True)
    xs = dev(ctx, x.reshape(nf, k * S))
    a = host(ctx.rx_demod(xs, k))
    assert ctx.last_dispatch() == fast_rx
    b = host(ctx.rx_demod(xs, k, out=_misaligned_u8(ctx, nf, k * ctx.bytes_per_symbol)))
    assert ctx.last_dispatch() == "k_sym<demod>"
    for got, what in ((a, fast_rx), (b, "k_sym")):
        assert_bytes_match(bytes(got.ravel()), want, wsoft, mod, what=what)
    # ---- TX symbol stream
    n_sym = 9
    nb = n_sym * ctx.bytes_per_symbol - 5
    stream = rng.integers(0, 256, nb, dtype=np.uint8)
    sd = torch.from_numpy(stream.copy()).to(ctx.device)
    nd = ctx.data_carriers
    opts = np.asarray(orc.modulate(bytes(stream), mod))
    pts = np.zeros(n_sym * nd, np.complex128); pts[: opts.size] = opts
    wtx = np.stack([orc.prefix_block(orc.encode_block(pts[i * nd:(i + 1) * nd], n, guard)[0]) for i in range(n_sym)])
    a = host(ctx.tx_symbols(sd, n_sym=n_sym))
    assert ctx.last_dispatch() == fast_tx
    b = host(ctx.tx_symbols(sd, n_sym=n_sym, out=_misaligned_c64(ctx, n_sym, S)))
    assert ctx.last_dispatch() == "k_sym<tx>"
    assert rel_err(a, wtx) < TOL and rel_err(b, wtx) < TOL
    # ---- encode
    nbytes = 300 if n == 64 else 900
    pay = rng.integers(0, 256, (3, nbytes), dtype=np.uint8)
    pd = torch.from_numpy(pay).to(ctx.device)
    a = host(ctx.encode_batch(pd))
    assert ctx.last_dispatch() == fast_enc
    b = host(ctx.encode_batch(pd, out=_misaligned_c64(ctx, 3, ctx.frame_samples(nbytes))))
    assert ctx.last_dispatch() == "k_sym<tx>+k_tx_finish"
    for f in range(3):
        wf = orc.encode(bytes(pay[f]), guard, mod, n)
        assert rel_err(a[f], wf) <= TOL and rel_err(b[f], wf) <= TOL
    # ---- the A/B switches route to the generic kernels as well, per context
    for key in ("no_fast64", "no_mid_kernels", "no_demod4096", "no_txframe64"):
        ctx.set_tuning(key, 1)
    c = host(ctx.rx_demod(xs, k))
    assert ctx.last_dispatch() == "k_sym<demod>"
    assert_bytes_match(bytes(c.ravel()), want, wsoft, mod, what="tuned off")
    with pytest.raises(api.OfdmError):
        ctx.set_tuning("no_such_key", 1)
    with pytest.raises(api.OfdmError):
        ctx.set_tuning("debug_demod64", 1)        # the ablation branches exist in the profile build only
    assert ctx.get_tuning("profile_build") == 0 and ctx.get_tuning("no_fast64") == 1


# ------------------------------------------------------------------ a24: channel (src/channel.rs:33-74) on the GPU
def test_channel_batch_matches_the_oracle(api, orc):
    """ofdm_channel_batch against orc_channel with the same SplitMix64 streams: FIR CHANNEL, CFO exp(+j f (i+1)) with
    f = pi U(0,1)/80, uniform noise scaled by the COMPLEX pseudo-variance; the drawn CFO bit for bit, samples <= 1e-6
    (f32 output of an f64 computation)."""
    rng = np.random.default_rng(24)
    ctx = api.Context(modulation=api.QPSK)
    frames = np.stack([orc.encode(bytes(rng.integers(0, 256, 400, dtype=np.uint8)), False, orc.QPSK) for _ in range(5)])
    x32 = fc32(frames)
    for snr, te in ((30.0, False), (30.0, True), (12.5, True)):
        y, fd = ctx.channel_batch(dev(ctx, x32), snr_db=snr, timing_error=te, seed=77, want_f_delta=True)
        y, fd = host(y), host(fd)
        assert y.shape == (5, frames.shape[1] + 63)
        for f in range(5):
            want, wfd = orc.channel(wide(x32[f]), snr, te, seed=77 + f)
            assert fd[f] == wfd
            assert rel_err(y[f], want) <= 1e-6
    # the MATLAB listing of conv((1-1i) ones(16), CHANNEL) (channel.rs:99-177), noise pushed below f32 resolution
    ones = np.full((1, 16), 1 - 1j, np.complex64)
    y = host(ctx.channel_batch(dev(ctx, ones), snr_db=300.0))[0]
    want = orc.convolve(wide(ones[0]), orc.channel_taps())
    assert rel_err(y, want) <= 1e-6
    assert abs(y[8].real - (-0.1912)) < 3e-4 and abs(y[9].real - 0.7404) < 3e-4 and abs(y[10].real - 1.0225) < 3e-4
    # taps table = the reference's
    taps = np.zeros(64)
    assert ctx.lib.ofdm_channel_taps(taps.ctypes.data) == 0
    np.testing.assert_array_equal(taps, orc.channel_taps())


def test_channel_batch_placement_and_cfo_override(api, orc):
    """The test-bench extensions: per-frame delay inside a longer slot, explicit (signed) CFO.  With the noise pushed
    below f32 resolution the slot equals the oracle's noiseless channel output shifted by the delay; with noise on, the
    samples outside the channel output carry noise only and the whole chain decodes (config-3 synthesis)."""
    import torch
    rng = np.random.default_rng(25)
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    pays = rng.integers(0, 256, (6, 560), dtype=np.uint8)
    tx = ctx.encode_batch(dev(ctx, pays))
    delay = torch.tensor([0, 1, 17, 33, 64, 5], dtype=torch.int32)
    fd = torch.tensor([0.0, 0.01, -0.02, 0.035, -0.037, 0.0], dtype=torch.float64)
    span = 2176
    y = host(ctx.channel_batch(tx, snr_db=300.0, seed=3, delay=delay, f_delta=fd, span=span))
    txh = host(tx)
    for f in range(6):
        c = np.convolve(wide(txh[f]), orc.channel_taps())[: txh.shape[1] + 63]
        c = c * np.exp(1j * float(fd[f]) * np.arange(1, c.size + 1))
        want = np.zeros(span, np.complex128)
        d = int(delay[f])
        m = min(c.size, span - d)
        want[d:d + m] = c[:m]
        assert rel_err(y[f], want) <= 1e-6
    y = ctx.channel_batch(tx, snr_db=30.0, seed=4, delay=delay, f_delta=fd, span=span)
    yh = host(y)
    assert np.all(np.abs(yh[2][:17]) > 0) and np.abs(yh[2][:17]).max() < 0.05     # noise only before the frame
    res = ctx.decode_batch(y, max_symbols=ctx.data_symbols(560))
    st = host(res["status"])
    assert np.all(st == 0)
    for f in range(6):
        w = orc.decode_sc(wide(yh[f]), True, orc.QAM64, 64, max_symbols=16)
        assert host(res["offset"])[f] == w["offset"] and abs(host(res["f_delta"])[f] - w["f_delta"]) <= 1e-9
        assert abs(host(res["f_delta"])[f] - float(fd[f])) < 2e-3               # the estimate tracks the injected CFO


def test_loopback_through_the_gpu_channel(api, orc):
    """examples/lab3a.rs / lab3b.rs entirely on the GPU: encode! -> channel! -> decode! (QPSK, no guard bands, 30 dB)."""
    data = bytes((i * 11 + 5) % 253 for i in range(400))
    tx = api.encode(data, False, api.QPSK)
    for te in (False, True):
        rx = api.channel(tx, 30.0, te, seed=9)
        assert rx.size == tx.size + 63
        got = api.decode(rx, False, api.QPSK, cfo_mode=api.CFO_ABS)
        assert got == data and orc.analysis(data, got) == (0, 0, 0.0)


def test_decode_errors(api, orc):
    # "Input not long enough, bailing early" (receiver.rs:27-29) and no-sync
    rng = np.random.default_rng(4)
    tx = orc.encode(b"hello world", False, orc.BPSK)
    with pytest.raises(api.DecodeError, match="Input not long enough"):
        api.decode(through_channel(orc, rng, tx[:700], 800, 3, 0.0, 30.0))
    with pytest.raises(api.DecodeError):
        api.decode(np.zeros(3000, np.complex64))


# ------------------------------------------------------------------ reference-shaped loop-back (examples/lab3a.rs, lab3b.rs)
@pytest.mark.parametrize("timing_error", [False, True])
def test_loopback_lab3_on_gpu(api, orc, timing_error):
    data = bytes((i * 7 + 3) % 251 for i in range(400))
    tx = api.encode(data, False, api.QPSK)            # ofdm::encode!(data, guard_bands, modulation)
    assert tx.size == 2880
    assert rel_err(tx, orc.encode(data, False, orc.QPSK)) <= TOL
    rx, fd = orc.channel(tx, 30.0, timing_error, seed=21)  # channel.rs restated with a seeded PRNG
    got = api.decode(rx, False, api.QPSK, cfo_mode=api.CFO_ABS)
    assert got == data
    assert orc.analysis(data, got) == (0, 0, 0.0)


# ------------------------------------------------------------------ size-independent properties at large sizes
def test_stdrng_pilot_tables(api, orc):
    """8(f) rank 3: contexts built with the restated rand-0.8 StdRng tables (transmitter.rs:75-96); unverified against a
    running `rand`, but the path must work with them exactly as with any other table."""
    rng = np.random.default_rng(77)
    pre, trn = api.stdrng_pilots(64)
    np.testing.assert_array_equal(pre, orc.stdrng_preamble(80))
    np.testing.assert_array_equal(trn, orc.stdrng_training(64))
    pay = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    tx = api.encode(pay, True, api.QAM64, pilots="stdrng")
    assert rel_err(tx, orc.encode(pay, guard=True, modulation=orc.QAM64, preamble=pre, training=trn)) < TOL
    assert rel_err(tx[80:160], tx[160:240]) == 0 and rel_err(tx, api.encode(pay, True, api.QAM64)) > 0.1  # other tables
    cap = through_channel(orc, rng, wide(fc32(tx)), 2400, 31, 0.004, snr_db=35.0, data_start=800)
    assert api.decode(wide(cap), True, api.QAM64, pilots="stdrng") == pay
    assert bytes(orc.decode_sc(wide(cap), guard=True, modulation=orc.QAM64, training=trn)["bytes"]) == pay


def test_outer_rs_over_the_link(api, orc):
    """8(f) rank 4 / lab3c wiring: text -> create_transmission_bytes -> encode -> channel -> decode ->
    decipher_transmission_bytes (src/utils.rs:97-180, examples/lab3c.rs:15-54), with two OFDM symbols blanked on the air:
    12 consecutive wrong-ish bytes inside one 255-byte block, which RS(255,223) repairs."""
    rng = np.random.default_rng(12)
    text = bytes(rng.integers(32, 127, 500, dtype=np.uint8))
    coded = api.create_transmission_bytes(text)
    assert len(coded) == 765 and coded == orc.create_transmission_bytes(text)
    tx = api.encode(coded, True, api.BPSK)
    assert tx.size == 800 + 80 * 131  # 765 B BPSK/guard -> 131 data symbols
    cap = wide(through_channel(orc, rng, tx, tx.size + 200, 40, 0.002, snr_db=30.0, data_start=800))
    start = 40 + 9 + 800 + 80 * 20
    cap[start:start + 160] = 0
    got = api.decode(cap, True, api.BPSK)
    assert len(got) == 765 and got != coded
    plain = api.decipher_transmission_bytes(got)
    assert plain is not None and plain[:500] == text == orc.decipher_transmission_bytes(got)[:500]
    cap[start:start + 80 * 8] = 0  # 48 bytes gone: beyond 16 per block -> None, like the reference
    assert api.decipher_transmission_bytes(api.decode(cap, True, api.BPSK)) is None


def test_lab3c_image_fixture_over_the_link_on_gpu(api, orc):
    """examples/lab3c_image.rs with the reference's own payload (support/dancing.bytes -> tests/golden/dancing.bytes, data): bytes ->
    create_transmission_bytes -> encode!(guard_bands) -> [fc32 file format] -> channel -> decode!(guard_bands) ->
    decipher_transmission_bytes == the image, on the GPU back-end, sample-for-sample and byte-for-byte against the oracle."""
    import os
    img = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dancing.bytes"), "rb").read()
    assert len(img) == 576
    coded = api.create_transmission_bytes(img)
    assert coded == orc.create_transmission_bytes(img) and len(coded) == 765
    tx = api.encode(coded, True)                                   # modulation defaults to BPSK (transmitter.rs:16-17)
    assert tx.size == 800 + 80 * 131 and rel_err(tx, orc.encode(coded, True, orc.BPSK)) <= TOL
    wire = api.sig_to_bytes(tx)                                    # utils::sig_to_bytes: what --transmit writes (fc32)
    rx, _ = orc.channel(api.bytes_to_sig(wire), 30.0, True, seed=24)
    for sync in ({}, {"sync_mode": api.SYNC_REFERENCE}):           # Schmidl-Cox timing and the reference's xcorr_fft timing
        got = api.decode(rx, True, cfo_mode=api.CFO_ABS, **sync)
        assert got == coded
        plain = api.decipher_transmission_bytes(got)
        assert plain is not None and plain[:576] == img == orc.decipher_transmission_bytes(got)[:576]
    assert orc.analysis(coded, got) == (0, 0, 0.0)


@pytest.mark.parametrize("n,mod,guard", [(64, 6, True), (64, 1, False), (256, 4, True), (1024, 6, True), (4096, 8, True)])
def test_tx_symbols_fused_equals_staged(api, orc, n, mod, guard):
    """ofdm_tx_symbols_batch = modulate + encode_block + prefix_block (transmitter.rs:40-53) in one pass: the samples of the
    three staged calls within 1e-5 (the fused call runs the R x 64 two-stage kernels, the staged ones the Stockham
    passes) and the oracle's within 1e-5."""
    import torch
    rng = np.random.default_rng(n + mod)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    bps = ctx.bytes_per_symbol
    nb = 5 * bps + bps // 3 + 1                      # the last symbol is only partly filled
    data = rng.integers(0, 256, nb, dtype=np.uint8)
    d = torch.from_numpy(data.copy()).to(ctx.device)
    fused = ctx.tx_symbols(d, n_sym=7)               # 6 symbols carry bytes, the 7th only pilots
    pts = ctx.modulate(d)
    nd = ctx.data_carriers
    padded = torch.zeros(7 * nd, dtype=torch.complex64, device=ctx.device)
    padded[: pts.numel()] = pts
    staged = ctx.prefix_block(ctx.encode_block(padded.view(7, nd)))
    # R x 64 two-stage kernels (k_tx_mid / k_tx4096) against the Stockham passes of the staged calls
    assert rel_err(host(fused), host(staged)) < TOL
    want = []
    opts = orc.modulate(bytes(data), mod)
    for sidx in range(7):
        blk, _ = orc.encode_block(opts[sidx * nd:(sidx + 1) * nd], n, guard)
        want.append(orc.prefix_block(blk))
    assert rel_err(host(fused), np.stack(want)) < TOL


@pytest.mark.parametrize("n,mod,guard,nbytes", [(256, 6, True, 2500), (1024, 4, True, 2500), (2048, 6, False, 9000)])
def test_tx_encode_build_once_variant_is_bit_identical(api, orc, n, mod, guard, nbytes):
    """Tuning txframe_rewrite = 1 (every symbol built once, unnormalised samples out, rescale sweep over what was just written --
    measured 5-12 % slower than building twice, kept as an A/B switch): the same two roundings per sample as the
    two-pass kernel, so the frames are bit-identical, ragged lengths and several frames per workgroup round included."""
    import torch

    rng = np.random.default_rng(n + mod)
    nfr = 11
    pay = rng.integers(0, 256, (nfr, nbytes), dtype=np.uint8)
    lens = rng.integers(0, nbytes + 1, nfr).astype(np.int32)
    lens[0], lens[1] = nbytes, 0
    a = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 3})
    b = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"grid_cap": 3, "txframe_rewrite": 1})
    fa = a.encode_batch(dev(a, pay), lens=torch.from_numpy(lens))
    fb = b.encode_batch(dev(b, pay), lens=torch.from_numpy(lens))
    assert a.last_dispatch() == "k_txframe_mid" and b.last_dispatch() == "k_txframe_mid<rewrite>"
    assert np.array_equal(host(fa).view(np.uint32), host(fb).view(np.uint32))
    want = orc.encode(bytes(pay[0]), guard, mod, n)
    assert rel_err(host(fb)[0][: want.size], want) <= TOL


@pytest.mark.parametrize("n,mod,guard", [(64, 6, True), (64, 2, False), (256, 4, True)])
def test_tx_encode_ragged_lengths(api, orc, n, mod, guard):
    """ofdm_tx_encode_batch with per-frame payload lengths (payload_len_dev): every frame occupies the slot of the longest
    payload; up to its own last data symbol it equals the oracle's frame for that payload (the pilot-only tail symbols
    are far below the frame maximum, so the normalisation is the same), and it decodes to its own length."""
    import torch
    rng = np.random.default_rng(n + mod)
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    maxb = 300
    lens = [300, 0, 1, 137, 299, 300]
    pay = rng.integers(0, 256, (len(lens), maxb), dtype=np.uint8)
    frames = host(ctx.encode_batch(torch.from_numpy(pay).to(ctx.device), lens=torch.tensor(lens, dtype=torch.int32)))
    S = ctx.S
    for f, ln in enumerate(lens):
        want = orc.encode(bytes(pay[f, :ln]), guard, mod, n)
        assert rel_err(frames[f][: want.size], want) < TOL, f"frame {f} (len {ln})"
        tail = frames[f][want.size:]
        assert tail.size % S == 0 and (tail.size == 0 or np.abs(tail).max() <= np.abs(frames[f][: want.size]).max())
        cap = through_channel(orc, rng, wide(frames[f]), frames[f].size + 120, 33, 0.003, snr_db=40.0, data_start=10 * S)
        assert api.decode(wide(cap), guard, mod, n_fft=n) == bytes(pay[f, :ln])


def test_set_stream_and_memset(api, orc):
    """ofdm_set_stream: the context enqueues on whatever HIP stream the host hands it (here a torch side stream);
    ofdm_memset: device fill on that stream."""
    import ctypes as C
    import torch
    ctx = api.Context(modulation=api.QAM64, guard_bands=True)
    side = torch.cuda.Stream(device=ctx.device)
    rng = np.random.default_rng(3)
    x, data = make_symbols(orc, rng, 16, 64, True, 6)
    with torch.cuda.stream(side):
        xd = ctx.to_device(x).view(1, -1)
        out = torch.empty((1, 16 * ctx.bytes_per_symbol), dtype=torch.uint8, device=ctx.device)
        ctx._ck(ctx.lib.ofdm_set_stream(ctx.h, C.c_void_p(side.cuda_stream)), "set_stream")
        ctx._ck(ctx.lib.ofdm_memset(ctx.h, C.c_void_p(out.data_ptr()), 0xA5, out.numel()), "memset")
        side.synchronize()
        assert bool((out == 0xA5).all())
        ctx.rx_demod(xd, syms_per_frame=16, out=out)
        ctx.synchronize()                       # ofdm_synchronize waits on the context's (= side) stream
    assert bytes(out.cpu().numpy()[0]) == orc.rx_demod(wide(x), 64, True, orc.QAM64) == data
    ctx._ck(ctx.lib.ofdm_set_stream(ctx.h, None), "set_stream")   # back to the device's default stream
    assert bytes(ctx.rx_demod(xd, syms_per_frame=16).cpu().numpy()[0]) == data
    assert ctx.lib.ofdm_set_stream(None, None) == -1 and ctx.lib.ofdm_memset(ctx.h, None, 0, 8) == -1


def test_large_batch_properties(api, orc):
    """Properties that need no oracle run, at sizes far beyond what the oracle finishes in seconds:
    TX -> RX round trip is the identity on bytes, two independent kernels (wave-centric fast path and the generic
    Stockham kernel) agree bit for bit, FFT linearity, and Schmidl-Cox timing is shift-equivariant."""
    import torch
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    g = torch.Generator(device=ctx.device); g.manual_seed(7)
    F, syms = 131072, 16   # 262144 groups = 16384 store bursts of 16: twice the persistent grid of k_demod64 (8192 wavefronts)
    nb = syms * ctx.bytes_per_symbol
    pay = torch.randint(0, 256, (F * nb,), dtype=torch.uint8, device=ctx.device, generator=g)
    x = ctx.prefix_block(ctx.encode_block(ctx.modulate(pay).view(-1, ctx.data_carriers))).view(F, syms * 80)
    x = x + torch.view_as_complex(torch.randn((F, syms * 80, 2), device=ctx.device, generator=g) * 0.001)  # sigma 0.008 per bin after the FFT: 18 sigma to a boundary
    fast = ctx.rx_demod(x, syms_per_frame=syms)                                  # k_demod64 (syms % 8 == 0)
    assert torch.equal(fast.view(-1), pay)                                       # round trip: BER 0
    generic = ctx.rx_demod(x.view(F * 4, 4 * 80), syms_per_frame=4)              # k_sym<64, DEMOD>
    assert torch.equal(generic.view(-1), fast.view(-1))                          # checksum of checksums: all bytes
    # linearity of the batched FFT at 1M vectors
    a = torch.view_as_complex(torch.randn((1 << 20, 64, 2), device=ctx.device, generator=g))
    b = torch.view_as_complex(torch.randn((1 << 20, 64, 2), device=ctx.device, generator=g))
    lhs = ctx.fft(a + 2 * b)
    rhs = ctx.fft(a) + 2 * ctx.fft(b)
    assert float((lhs - rhs).abs().max() / rhs.abs().max()) < 1e-5
    assert float((ctx.fft(ctx.fft(a), inverse=True) - a).abs().max()) < 1e-4    # ifft(fft(x)) == x
    # Schmidl-Cox: delaying the capture by k samples moves d_hat by k (same CFO, same metric)
    rng = np.random.default_rng(3)
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64)
    base = through_channel(orc, rng, tx, 2176, 10, 0.02, 30.0)
    shifts = np.arange(0, 40, 2)
    caps = np.stack([np.concatenate([np.zeros(k, np.complex64), base[: 2176 - k]]) for k in shifts])
    d, fd, m = (host(t) for t in ctx.sc_correlate(dev(ctx, caps)))
    assert np.array_equal(d - d[0], shifts) and np.abs(fd - fd[0]).max() < 1e-6


def test_edge_cases(api, orc):
    import torch
    # empty payload: header only (one data symbol), on both sides of the link
    for mod, guard in ((api.BPSK, False), (api.QAM64, True)):
        ctx = api.Context(modulation=mod, guard_bands=guard)
        frames = ctx.encode_batch(torch.zeros((2, 0), dtype=torch.uint8, device=ctx.device))
        want = orc.encode(b"", guard, mod)
        assert frames.shape[1] == want.size and rel_err(host(frames)[0], want) <= TOL
        cap = np.concatenate([np.zeros(7, np.complex64), host(frames)[0], np.zeros(120, np.complex64)])
        res = ctx.decode_batch(dev(ctx, cap).reshape(1, -1), max_symbols=ctx.data_symbols(0))
        assert int(res["status"][0]) == 0 and int(res["len"][0]) == 0
        short = ctx.decode_batch(dev(ctx, cap).reshape(1, -1), max_symbols=1)  # BPSK: 8 bytes/symbol < 16-byte header
        assert int(short["status"][0]) == (api.FRAME_HEADER if mod == api.BPSK else 0)
    # ragged batch: frames of different true length in equal slots -> per-frame status / length
    ctx = api.Context(modulation=api.QPSK)
    rng = np.random.default_rng(9)
    slot = 4000
    caps, pays = [], []
    for n in (0, 1, 100, 400, 399):
        pay = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        tx = orc.encode(pay, False, orc.QPSK)
        caps.append(through_channel(orc, rng, tx, slot, 5, 0.01, 35.0)); pays.append(pay)
    caps.append(fc32(0.01 * (rng.standard_normal(slot) + 1j * rng.standard_normal(slot)))); pays.append(None)   # noise only
    caps.append(np.concatenate([caps[3][:900], np.zeros(slot - 900, np.complex64)])); pays.append(None)             # truncated
    res = ctx.decode_batch(dev(ctx, np.stack(caps)), max_symbols=40, frame_len=slot)
    st, ln = host(res["status"]), host(res["len"])
    for f, pay in enumerate(pays):
        w = orc.decode_sc(wide(caps[f]), False, orc.QPSK, max_symbols=40)
        assert st[f] == w["status"], f
        if pay is not None:
            assert st[f] == 0 and ln[f] == len(pay) and bytes(host(res["bytes"])[f][: ln[f]]) == pay == w["bytes"]
    assert st[5] == api.FRAME_NOSYNC
    # maximum supported transform and the widest constellation through the whole chain once
    ctx = api.Context(n_fft=4096, modulation=api.QAM256, guard_bands=True)
    pay = rng.integers(0, 256, (1, 9000), dtype=np.uint8)
    frames = host(ctx.encode_batch(torch.from_numpy(pay).to(ctx.device)))
    assert rel_err(frames[0], orc.encode(bytes(pay[0]), True, orc.QAM256, 4096)) <= TOL


# ------------------------------------------------------------------ C++ host mirror (include/ofdm_host.hpp): lab3a / lab3b loop-back
def test_rx_decode_rejects_rows_too_short_for_the_outer_code(api, orc):
    """ofdm_rx_decode_batch must refuse an out_stride that cannot hold what the finish kernel may write -- also with
    Hamming(7,4) on, where a row needs floor((max_symbols * bytes_per_symbol - 16) / 7) * 4 bytes."""
    import ctypes as C
    import torch

    for ecc in (api.ECC_NONE, api.ECC_HAMMING74):
        ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, ecc=ecc)
        D = 16
        body = D * ctx.bytes_per_symbol - 16
        need = body if ecc == api.ECC_NONE else body // 7 * 4
        x = torch.zeros((2, 2176), dtype=torch.complex64, device=ctx.device)
        i32 = lambda: torch.zeros(2, dtype=torch.int32, device=ctx.device)
        for stride, ok in ((need, True), (need - 1, False), (0, False)):
            out = torch.zeros((2, max(need, 4)), dtype=torch.uint8, device=ctx.device)
            ln, st = i32(), i32()
            rc = ctx.lib.ofdm_rx_decode_batch(ctx.h, C.c_void_p(x.data_ptr()), 2, 2176, 2176, 0, D, C.c_void_p(out.data_ptr()),
                                              stride, C.c_void_p(ln.data_ptr()), C.c_void_p(st.data_ptr()), None, None, None)
            assert (rc == 0) == ok, (ecc, stride, rc)
        ctx.synchronize()


def test_two_contexts_interleaved_and_device_restored(api, orc):
    """Two contexts held by one thread, calls interleaved: each runs on its own context's device and leaves the thread's
    current device alone (DeviceGuard in every entry point; one GPU here, so both contexts share cuda:0)."""
    import torch

    rng = np.random.default_rng(12)
    a = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    b = api.Context(n_fft=1024, modulation=api.QPSK, guard_bands=False)
    xa, da = make_symbols(orc, rng, 16, 64, True, 6, 33.0)
    xb, db = make_symbols(orc, rng, 3, 1024, False, 2, 33.0)
    before = torch.cuda.current_device()
    oa = a.rx_demod(dev(a, xa).reshape(2, -1), 8)
    ob = b.rx_demod(dev(b, xb).reshape(1, -1), 3)
    oa2 = a.rx_demod(dev(a, xa).reshape(1, -1), 16)
    a.synchronize(); b.synchronize()
    assert torch.cuda.current_device() == before
    assert bytes(host(oa).ravel()) == da == bytes(host(oa2).ravel()) and bytes(host(ob).ravel()) == db


def test_cpp_host_loopback(ofdm):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "ofdm_loopback")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tools", "ofdm_loopback.cpp"), "-L", os.path.join(root, "ofdm_amd"), "-lofdm_hip",
                           "-Wl,-rpath," + os.path.join(root, "ofdm_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    for args in ([], ["--timing-error"], ["--guard", "--qam64", "--bytes", "560", "--timing-error"],
                 ["--pilots", "stdrng", "--timing-error"],
                 ["--ecc", "--bpsk", "--guard", "--bytes", "500", "--timing-error"]):   # lab3c: 500 B text -> RS -> 765 B
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.stdout, r.stderr)          # exit 0 <=> Analysis.num_errs == 0
        assert "num_errs: 0" in r.stdout and "I met a traveller" in r.stdout
    # frame-index split inside one process: N contexts (own stream, own host thread) == one context, byte for byte
    for n_ctx in (1, 2, 3):
        r = subprocess.run([exe, "--devices", str(n_ctx), "--frames", "37", "--guard", "--qam64", "--bytes", "560", "--timing-error"],
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0 and "identical to the single-context result" in r.stdout and "37 decoded, num_errs: 0" in r.stdout, (n_ctx, r.stdout, r.stderr)
    # fc32 file wire format + capture slicing (examples/lab3c.rs:15-54, src/utils.rs:228-254)
    import tempfile
    import numpy as np
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tx.fc32")
        r = subprocess.run([exe, "--transmit", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and os.path.getsize(path) == 2880 * 8          # 400 B QPSK frame, 8 B per sample
        tx = np.fromfile(path, dtype=np.float32).reshape(-1, 2)
        assert abs(max(tx[:, 0].max(), tx[:, 1].max()) - 1.0) < 1e-6            # normalised frame (transmitter.rs:183-194)
        cap = np.concatenate([np.zeros((1234, 2), np.float32), tx, np.zeros((777, 2), np.float32)])
        cap += np.random.default_rng(0).standard_normal(cap.shape).astype(np.float32) * 1e-3
        cpath = os.path.join(td, "rx.fc32")
        cap.tofile(cpath)
        for extra in ([], ["--start", "1000", "--stop", "4700"]):
            r = subprocess.run([exe, "--receive", cpath] + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and "received 400 bytes" in r.stdout, (extra, r.stdout)
        # a long capture file (the 2 M-sample buffers of examples/jetson_rx.rs, here 600 000 samples with the frame at 412 345): the C++
        # host's decode goes through ofdm_rx_decode_long_host, i.e. the slice search
        rng = np.random.default_rng(1)
        long_cap = (rng.standard_normal((600_000, 2)) * 1e-3).astype(np.float32)
        long_cap[412_345:412_345 + tx.shape[0]] += tx
        lpath = os.path.join(td, "long.fc32")
        long_cap.tofile(lpath)
        r = subprocess.run([exe, "--receive", lpath], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "received 400 bytes" in r.stdout, r.stdout


# ------------------------------------------------------------------ the generic kernel's persistent loop, every mode
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_k_sym_many_steps_per_workgroup_change_nothing(api, orc, n):
    """k_sym<N, MODE> is a persistent kernel: a workgroup takes G = 256 / (N / 8) symbols (frames for the channel estimate) per step
    and strides over the batch, with the next step's samples / payload dwords fetched a step ahead and its LDS staging reused.  The
    device-sized grid gives every workgroup ONE step on any batch a test can afford, so every mode runs here on grids of 1 and 3
    workgroups too (tuning key grid_cap), on batches of more than eight steps whose last step is partial: the same arithmetic per
    symbol whatever the grid, so the results must be the same bits as the device-sized grid's, which the tests above hold against
    the oracle.  The shape-specialised kernels are switched off by their tuning keys and every call asserts its dispatch."""
    import torch
    rng = np.random.default_rng(9000 + n)
    S = n + n // 4
    G = max(1, 256 // (n // 8))
    total = 8 * G + max(1, G // 2)
    assert total > 8 * G and (G == 1 or total % G)
    mod, guard = 6, True
    ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard, tuning={"no_fast64": 1, "no_mid_kernels": 1, "no_demod4096": 1, "no_txframe64": 1})

    def cx(*shape):
        return dev(ctx, fc32(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)))

    bins, blocks = cx(total, n), cx(total, S)
    D = 3
    F = next(f for f in range(-(-total // D), 4 * total) if G == 1 or (f * D) % G)
    x, _ = make_symbols_np(orc, rng, F * D, n, guard, mod, snr_db=20.0)
    xs, hks = dev(ctx, x.reshape(F, D * S)), cx(F, n)
    caps = cx(total, 10 * S + 40)
    offs = torch.from_numpy(rng.integers(0, 60, total).astype(np.int32)).to(ctx.device)
    fds = torch.from_numpy((rng.random(total) * 1.6 - 0.8) * np.pi / S).to(ctx.device)
    stream = torch.from_numpy(rng.integers(0, 256, total * ctx.bytes_per_symbol - 5, dtype=np.uint8)).to(ctx.device)
    nbytes = 2 * ctx.bytes_per_symbol                                # 16-byte header + body: three data symbols per frame
    assert ctx.data_symbols(nbytes) == D
    pay = torch.from_numpy(rng.integers(0, 256, (F, nbytes), dtype=np.uint8)).to(ctx.device)
    lens = torch.from_numpy(rng.integers(0, nbytes + 1, F).astype(np.int32))
    calls = [
        ("k_sym<fft>", lambda: ctx.fft(bins)),
        ("k_sym<ifft>", lambda: ctx.fft(bins, inverse=True)),
        ("k_sym<fft>", lambda: ctx.unprefix_block(blocks)),         # the same kernel reading past a cyclic prefix
        ("k_sym<ifft_cp>", lambda: ctx.prefix_block(bins)),
        ("k_sym<demod>", lambda: torch.cat([t.view(torch.uint8).reshape(-1) for t in ctx.rx_demod(xs, D, hk=hks, want_soft=True)])),
        ("k_sym<demod>", lambda: ctx.rx_demod(xs, D - 1, first_symbol=1, frame_len=D * S - S // 2)),
        ("k_sym<chest>", lambda: ctx.estimate_channel(caps, offs, fds, frame_len=10 * S + 20)),
        ("k_sym<tx>", lambda: ctx.tx_symbols(stream, n_sym=total)),
        ("k_sym<tx>+k_tx_finish", lambda: ctx.encode_batch(pay, out=_misaligned_c64(ctx, F, ctx.frame_samples(nbytes)), lens=lens)),
    ]

    def raw(t):                                                      # the bits: -0.0 is not 0.0 here
        return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t

    for i, (name, call) in enumerate(calls):
        outs = []
        for cap in (0, 1, 3):
            ctx.set_tuning("grid_cap", cap)
            outs.append(raw(call()))
            assert ctx.last_dispatch() == name, (i, cap, ctx.last_dispatch())
        ctx.synchronize()
        assert bool(outs[0].any()), (n, i, name)
        for cap, o in zip((1, 3), outs[1:]):
            assert torch.equal(o, outs[0]), (n, i, name, cap)
