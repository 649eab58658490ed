"""GPU checks of the soft-decision receive path (OFDM_ECC_HAMMING74_SOFT, ofdm_rx_llr_batch, ofdm_hamming74_decode_soft) against the
numpy restatement tests/soft_ref.py and against the hard-decision chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_ref as sr  # noqa: E402
from chain_checks import assert_chunking_changes_nothing, assert_entry_points_agree, ofdm_api as _api  # noqa: E402
from chain_refs import soft_reference_decode  # noqa: E402
from tools.link import bit_errors, data_snr as _data_snr, link_on  # noqa: E402

pytestmark = pytest.mark.gpu

MODS = (1, 2, 4, 6, 8)


def _data_bins(orc, n, guard):
    return np.array([i for i in range(n) if orc.carrier_class(i, n, guard) == 0])


def _noisy_symbols(ctx, g, n_frames, syms, sigma):
    nb = n_frames * syms * ctx.bytes_per_symbol
    data = torch.randint(0, 256, (nb,), dtype=torch.uint8, device=ctx.device, generator=g)
    x = ctx.tx_symbols(data, n_sym=n_frames * syms).reshape(n_frames, syms * ctx.S)
    amp = float(x.abs().pow(2).mean().sqrt())
    noise = torch.randn((n_frames, syms * ctx.S, 2), device=ctx.device, generator=g) * (sigma * amp)
    return (x + torch.view_as_complex(noise)).contiguous()


# ---------------------------------------------------------------------------------------------------------- 1. LLRs
@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
def test_llr_matches_the_restatement(orc, n):
    api = _api()
    g = torch.Generator(device="cuda"); g.manual_seed(n)
    F, D = 3, 2
    total = exact = 0
    for guard in (False, True):
        bins = _data_bins(orc, n, guard)
        for mod in MODS:
            ctx = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
            x = _noisy_symbols(ctx, g, F, D, 0.03)
            h_frame = (1.0 + 0.3 * torch.view_as_complex(torch.randn((F, n, 2), device=ctx.device, generator=g))).to(torch.complex64)
            for hk in (h_frame.contiguous(), h_frame[0].contiguous(), None):
                hard, soft = ctx.rx_demod(x, D, hk=hk, want_soft=True)
                L = ctx.rx_llr(x, D, hk=hk)
                ctx.synchronize()
                pts = soft.cpu().numpy().reshape(F, D, -1)
                w = None if hk is None else sr.channel_weights(hk.cpu().numpy().reshape(-1, n), bins)
                want = sr.frame_llrs(pts, mod, api.SOFT_LLR_SCALE, w)
                got = L.cpu().numpy()
                assert got.shape == want.shape == (F, D * len(bins) * mod)
                d = np.abs(got.astype(np.int32) - want.astype(np.int32))
                assert d.max() <= 1, (n, guard, mod, hk is None)
                total += d.size
                exact += int((d == 0).sum())
                bits = sr.unpack_bits(hard.cpu().numpy())
                strong = np.abs(got) >= 1
                assert ((got > 0) == (bits == 1))[strong].all(), (n, guard, mod)     # positive means bit 1
                if hk is not None:   # a channel with 4x the gain: same equalised points, same w, same L
                    assert torch.equal(ctx.rx_llr((x * 4.0).contiguous(), D, hk=(hk * 4.0).contiguous()), L)
    assert exact >= 0.999 * total, (exact, total)


def test_llr_argument_checks():
    api = _api()
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    x = torch.zeros((1, 80), dtype=torch.complex64, device=ctx.device)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.OfdmError):
            ctx.rx_llr(x, 1, scale=bad)
    out = torch.empty((1, 48 * 4), dtype=torch.int8, device=ctx.device)
    rc = ctx.lib.ofdm_rx_llr_batch(ctx.h, x.data_ptr(), 1, 80, 80, 0, 1, None, None, None, 0, 16.0, out.data_ptr(), 48 * 4 - 1)
    assert rc == -1


# ---------------------------------------------------------------------------------------------------------- 2. the soft decoder
def test_soft_decoder_is_ml_on_random_llrs():
    api = _api()
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_HAMMING74_SOFT)
    rng = np.random.default_rng(7)
    parts = [rng.integers(-127, 128, 56 * 4000), rng.integers(-2, 3, 56 * 4000), np.zeros(56 * 8, np.int64),
             rng.choice([-127, 127, 0], 56 * 1000), rng.choice([-5, 5], 56 * 1000)]
    llr = np.concatenate(parts).astype(np.int8)
    for off, n_bits in ((0, llr.size), (3, llr.size - 60), (8, 56 * 7 + 30)):  # aligned, unaligned start, a ragged tail
        src = torch.from_numpy(llr).to(ctx.device)[off:off + n_bits]
        got = ctx.hamming74_decode_soft(src.contiguous() if off % 8 == 0 else src)
        ctx.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), sr.ham_decode_soft(llr[off:off + n_bits]))


def test_equal_magnitude_llrs_give_the_syndrome_decoder():
    api = _api()
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_HAMMING74_SOFT)
    rng = np.random.default_rng(8)
    data = torch.from_numpy(rng.integers(0, 256, 4 * 5000, dtype=np.uint8)).to(ctx.device)
    code = ctx.hamming74_encode(data)
    bits = sr.unpack_bits(code.cpu().numpy())
    flips = rng.random(bits.size) < 0.08
    rx = bits ^ flips
    rx_bytes = torch.from_numpy(np.packbits(rx, bitorder="little")).to(ctx.device)
    want, _ = ctx.hamming74_decode(rx_bytes)
    got = ctx.hamming74_decode_soft(torch.from_numpy(((2 * rx.astype(np.int8) - 1) * 37).astype(np.int8)).to(ctx.device))
    ctx.synchronize()
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------- 3. transmit
def test_transmit_is_unchanged():
    api = _api()
    for n, mod in ((64, api.QAM64), (1024, api.QAM16)):
        h = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_HAMMING74)
        s = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_HAMMING74_SOFT)
        for nb in (0, 1, 560, 1304):
            assert (s.coded_len(nb), s.data_symbols(nb), s.frame_samples(nb)) == (h.coded_len(nb), h.data_symbols(nb), h.frame_samples(nb))
        pay = torch.randint(0, 256, (5, 777), dtype=torch.uint8, device=h.device)
        lens = torch.tensor([777, 0, 13, 500, 776], dtype=torch.int32)
        assert torch.equal(s.encode_batch(pay, lens=lens), h.encode_batch(pay, lens=lens))


# ---------------------------------------------------------------------------------------------------------- helpers of 4-8
def _link(n, mod, n_frames, payload, snr, seed, guard=True):
    """a hard and a soft Hamming context over ONE capture (the frames on the wire are the same): the seeded link of tools/link.py"""
    api = _api()
    h = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=api.ECC_HAMMING74)
    s = api.Context(n_fft=n, modulation=mod, guard_bands=guard, ecc=api.ECC_HAMMING74_SOFT)
    pay, rx = link_on(h, n_frames, payload, snr, seed)
    return h, s, pay, rx, h.data_symbols(payload)


def _same(a, b, keys=("status", "len", "offset", "f_delta", "metric")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------- 4. clean channel
@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
def test_clean_channel_soft_equals_hard(n):
    for i, mod in enumerate(MODS):
        payload = 300 + 37 * i
        # 30 dB on the data symbols; 256-QAM 38 dB: at 30 dB its 16-byte length header (hard bits, no code) breaks on faded carriers
        h, s, pay, rx, D = _link(n, mod, 4, payload, _data_snr(n, 38.0 if mod == 8 else 30.0), 100 * n + i)
        rh = h.decode_batch(rx, max_symbols=D)
        rs = s.decode_batch(rx, max_symbols=D)
        s.synchronize()
        _same(rh, rs)
        assert (rs["status"] == 0).all() and (rs["len"] == (payload + 3) // 4 * 4).all(), (n, mod)
        assert torch.equal(rs["bytes"][:, :payload], pay), (n, mod)
        hard_right = (rh["bytes"][:, :payload] == pay).all(dim=1)
        assert int(hard_right.sum()) >= 3, (n, mod)                      # a clean channel: the hard decoder is right too ...
        want = (payload + 3) // 4 * 4
        assert torch.equal(rs["bytes"][hard_right, :want], rh["bytes"][hard_right, :want]), (n, mod)   # ... and then the two agree


# ---------------------------------------------------------------------------------------------------------- 5. composition
@pytest.mark.parametrize("n,mod", [(64, 6), (256, 4), (1024, 6), (4096, 2)])
def test_chain_is_the_composition_of_the_stages(n, mod):
    h, s, pay, rx, D = _link(n, mod, 7, 400, _data_snr(n, 16.0), 5 + n)   # noisy: the soft decisions matter
    r = s.decode_batch(rx, max_symbols=D)
    hk = s.estimate_channel(rx, r["offset"], r["f_delta"])
    L = s.rx_llr(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
    s.synchronize()
    assert int((r["status"] == 0).sum()) >= 5
    ref = soft_reference_decode(s, rx, r, D)     # the length from the hard header bytes, the blocks from soft_ref over the same LLRs
    assert len(ref) >= 5
    for f in range(rx.shape[0]):
        if int(r["status"][f]) != 0:
            continue
        n_out = int(r["len"][f])
        want = s.hamming74_decode_soft(L[f, 128:128 + n_out // 4 * 56].contiguous())
        assert torch.equal(r["bytes"][f, :n_out], want), f
        assert (n_out, bytes(want.cpu().numpy())) == ref[f], f
    assert_chunking_changes_nothing(s, rx, D, r)   # many chunks of the LLR workspace: the same rows, byte for byte


# ---------------------------------------------------------------------------------------------------------- 6. soft beats hard
# (snr_db, N) points of the committed BER curve (profiles/soft_ber_and_speed.json, N = 64: hard 1.6e-3 / 4.9e-4 / 1.1e-4 payload BER at
# 12 / 14 / 16 dB, soft 3.9 to 9 times fewer errors) where hard decoding leaves far more than 50 payload bit errors in 1024 frames and
# at least 500 frames synchronise; soft must leave fewer at each, and at most half as many at one of them
SOFT_POINTS = ((12.0, 64), (14.0, 64), (16.0, 64))


def _payload_bit_errors(r, pay):
    ok = (r["status"] == 0) & (r["len"] == (pay.shape[1] + 3) // 4 * 4)
    return bit_errors(torch.bitwise_xor(r["bytes"][:, :pay.shape[1]], pay)[ok]), ok


def test_soft_beats_hard_at_low_snr():
    halves = False
    for snr, n in SOFT_POINTS:
        h, s, pay, rx, D = _link(n, 6, 1024, 560, snr, 9000 + int(snr))
        rh, rs = h.decode_batch(rx, max_symbols=D), s.decode_batch(rx, max_symbols=D)
        eh, okh = _payload_bit_errors(rh, pay)
        es, oks = _payload_bit_errors(rs, pay)
        assert torch.equal(okh, oks) and int(okh.sum()) >= 500, (snr, int(okh.sum()))
        assert eh >= 50, (snr, eh)
        assert es < eh, (snr, es, eh)
        halves |= 2 * es <= eh
    assert halves


# ---------------------------------------------------------------------------------------------------------- 7. entry points
def test_every_decode_entry_point_in_soft_mode():
    api = _api()
    h, s, pay, rx, D = _link(64, 6, 6, 560, 16.0, 77)
    r, ones = assert_entry_points_agree(api, s, rx, D, dict(ecc=api.ECC_HAMMING74_SOFT))
    assert [st for st, _, _, _ in ones] == [0] * 6                # api.decode was asked for every frame
    rt = api.decode(api.encode(b"soft decisions", True, api.QAM16, ecc=api.ECC_HAMMING74_SOFT), True, api.QAM16,
                    ecc=api.ECC_HAMMING74_SOFT)
    assert rt[:14] == b"soft decisions"


# ---------------------------------------------------------------------------------------------------------- 8. dispatch
@pytest.mark.parametrize("n", [64, 1024])
def test_dispatch_names_the_soft_kernels(n):
    h, s, pay, rx, D = _link(n, 6, 2, 300, 30.0, 3)
    s.decode_batch(rx, max_symbols=D)
    ds = s.last_dispatch()
    h.decode_batch(rx, max_symbols=D)
    dh = h.last_dispatch()
    assert "k_sym<llr>" in ds and "k_rx_finish_soft" in ds, ds
    assert "k_sym<llr>" not in dh and "soft" not in dh, dh
    s.rx_llr(rx, D, first_symbol=10)
    assert s.last_dispatch() == "k_sym<llr>"
