"""EXT-10 on the GPU: sc16 (int16 I/Q) transmit output and sc16 long captures.  Nothing here has a tolerance: row f of an sc16 encode is
ofdm_sc16_narrow of frame f of the fc32 encode on the same arguments, and an sc16 long decode returns what the fc32 call returns on the
widened capture -- both bit for bit.

References: tests/sc16_ref.py (the numpy definition, held to the host functions by tests/test_sc16_cpu.py) applied to the project's own
fc32 entry points.  Every shape encodes its fc32 frames once and narrows them per scale."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sc16_ref  # noqa: E402
from tools.link import link as _link  # noqa: E402

pytestmark = pytest.mark.gpu
SCALES = [32767.0, 12000.0, 30000 / 3.1, 40000.0]     # the last clips on every shape: a normalised frame's positive peak is 1
SENTINEL = 12345


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


def payload_for(ctx, D):
    """a payload size whose frame has D data symbols"""
    p = max(D * ctx.bytes_per_symbol - 16, 0)
    assert ctx.data_symbols(p) == D, (D, p, ctx.data_symbols(p))
    return p


def payloads(ctx, seed, n, p):
    import torch

    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, (n, max(p, 1)), dtype=np.uint8)[:, :p].copy()).to(ctx.device)


def ragged(ctx, p, n=5):
    import torch

    base = [0, 1, p // 2, max(p - 1, 0), p]
    return torch.tensor([min(base[f % 5], p) for f in range(n)], dtype=torch.int32, device=ctx.device)


def twin(ctx, pay, lens=None):
    """the fc32 frames of ofdm_tx_encode_batch on the host, and the dispatch string of that call"""
    fc = ctx.encode_batch(pay, lens=lens).cpu().numpy()
    return fc, ctx.last_dispatch()


def narrowed(fc, scale):
    """(int16 [n, frame, 2], [clipped per frame]) of fc32 frames: the definition, frame by frame"""
    rows = [sc16_ref.narrow(fc[f], scale) for f in range(fc.shape[0])]
    return np.stack([r[0] for r in rows]), [r[1] for r in rows]


def check(ctx, pay, lens, fc, scale, what, out=None):
    """encode_batch_sc16 against the narrowed twin: samples and counts equal -> (dispatch, counts)"""
    got, clipped = ctx.encode_batch_sc16(pay, scale, out=out, lens=lens, want_clipped=True)
    disp = ctx.last_dispatch()
    want, want_clipped = narrowed(fc, scale)
    frame = fc.shape[1]
    assert np.array_equal(got.cpu().numpy()[:, :frame], want), (what, scale, disp)
    assert clipped.cpu().numpy().tolist() == want_clipped, (what, scale, disp)
    return disp, want_clipped


def rows_view(flat, base, n, ln, stride):
    """int16 rows [n, ln, 2] of a flat [samples, 2] device tensor, row f starting at sample base + f * stride (a view)"""
    import torch

    return torch.as_strided(flat, (n, ln, 2), (2 * stride, 2, 1), 2 * base)


# ------------------------------------------------------------------ 1. the fused kernel
@pytest.mark.parametrize("guard", [False, True], ids=["full", "guard"])
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_fused_encode_is_the_narrowed_fc32_frame(api, mod, guard):
    """N = 64, every modulation with and without guard bands; D = the fewest data symbols the modulation allows, 8, 9, 33 (five 8-symbol
    groups on four wavefronts: the group loop wraps) and 56; 5 frames with lens [0, 1, p // 2, p - 1, p]; four scales."""
    ctx = api.Context(n_fft=64, modulation=mod, guard_bands=guard)
    clipped_at_40000 = 0
    for D in sorted({ctx.data_symbols(0), 8, 9, 33, 56}):
        p = payload_for(ctx, D)
        pay, lens = payloads(ctx, 3000 + 100 * mod + D, 5, p), ragged(ctx, p)
        fc, fc_disp = twin(ctx, pay, lens)
        assert fc_disp == "k_txframe64", fc_disp
        for scale in SCALES:
            disp, counts = check(ctx, pay, lens, fc, scale, (mod, guard, D))
            assert disp == "k_txframe64_sc16", disp
        assert all(k >= 1 for k in counts), counts          # 40000 > 32767 times a positive peak of 1
        clipped_at_40000 += sum(counts)
    assert clipped_at_40000 > 0


# ------------------------------------------------------------------ 2. the persistent grid
def test_persistent_grid_and_prefetch_past_the_batch(api):
    """64-QAM / guard / D = 16: 1, 3 and 70 frames under the device-sized grid and under grids of 1 and 3 workgroups (many frames per
    workgroup; the prefetch of the frame after next crosses the end of the batch); every frame also equals the same payload encoded alone."""
    import torch

    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    p = payload_for(ctx, 16)
    pay = payloads(ctx, 3100, 70, p)
    lens = torch.from_numpy(np.random.default_rng(3101).integers(0, p + 1, 70).astype(np.int32)).to(ctx.device)
    fc, _ = twin(ctx, pay, lens)
    want, want_clipped = narrowed(fc, 40000.0)
    for f in range(70):                                           # alone
        q, k = ctx.encode_batch_sc16(pay[f:f + 1], 40000.0, lens=lens[f:f + 1], want_clipped=True)
        assert np.array_equal(q.cpu().numpy()[0], want[f]) and int(k[0]) == want_clipped[f], f
    for cap in (0, 1, 3):
        ctx.set_tuning("grid_cap", cap)
        for n in (1, 3, 70):
            disp, _ = check(ctx, pay[:n], lens[:n], fc[:n], 40000.0, (cap, n))
            assert disp == "k_txframe64_sc16"
    ctx.set_tuning("grid_cap", 0)


# ------------------------------------------------------------------ 3. layout
def test_output_layouts_and_byte_wise_payload_rows(api):
    import torch

    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    p = payload_for(ctx, 9)
    n, frame = 5, ctx.frame_samples(p)
    pay, lens = payloads(ctx, 3200, n, p), ragged(ctx, p)
    fc, fc_disp = twin(ctx, pay, lens)
    scale = 30000 / 3.1

    def run(stride, base):
        flat = torch.full((base + n * stride + 8, 2), SENTINEL, dtype=torch.int16, device=ctx.device)
        disp, _ = check(ctx, pay, lens, fc, scale, (stride, base), out=rows_view(flat, base, n, frame, stride))
        keep = torch.ones(flat.shape[0], dtype=torch.bool, device=ctx.device)
        for f in range(n):
            keep[base + f * stride: base + f * stride + frame] = False
        assert bool((flat[keep] == SENTINEL).all()), ("wrote outside the frames", stride, base)
        return disp

    assert run(frame + 4, 0) == "k_txframe64_sc16"                               # rows apart, tails survive, still fused
    assert run(frame + 1, 0) == fc_disp + "+k_sc16_narrow"                       # a stride that is no multiple of 4 samples
    assert run(frame, 1) == fc_disp + "+k_sc16_narrow"                           # a base one sample off 16-byte alignment
    # payload rows at an odd base and an odd stride: k_txframe64's byte-wise payload path, fused
    stride = p + 3 if (p + 3) % 2 else p + 4
    raw = torch.zeros(1 + n * stride + p, dtype=torch.uint8, device=ctx.device)
    for f in range(n):
        raw[1 + f * stride: 1 + f * stride + p] = pay[f]
    out = torch.full((n, frame, 2), SENTINEL, dtype=torch.int16, device=ctx.device)
    clipped = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    rc = ctx.lib.ofdm_tx_encode_sc16_batch(ctx.h, raw.data_ptr() + 1, n, stride, lens.data_ptr(), p, scale, out.data_ptr(), frame,
                                           clipped.data_ptr())
    assert rc == 0 and ctx.last_dispatch() == "k_txframe64_sc16"
    want, want_clipped = narrowed(fc, scale)
    assert np.array_equal(out.cpu().numpy(), want) and clipped.cpu().numpy().tolist() == want_clipped


# ------------------------------------------------------------------ 4. outside the envelope: the fc32 chain + k_sc16_narrow
def test_more_than_56_data_symbols_take_the_two_pass_path(api):
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    p = payload_for(ctx, 57)
    pay, lens = payloads(ctx, 3300, 3, p), ragged(ctx, p, 3)
    fc, fc_disp = twin(ctx, pay, lens)
    assert "k_txframe64" not in fc_disp.split("+")
    for scale in (12000.0, 40000.0):
        disp, _ = check(ctx, pay, lens, fc, scale, "D = 57")
        assert disp == fc_disp + "+k_sc16_narrow", disp


@pytest.mark.parametrize("n_fft", [128, 1024, 4096])
def test_other_transform_lengths_take_the_two_pass_path(api, n_fft):
    ctx = api.Context(n_fft=n_fft, modulation=api.QAM16, guard_bands=True)
    p = 3 * ctx.bytes_per_symbol + 5
    pay, lens = payloads(ctx, 3400 + n_fft, 3, p), ragged(ctx, p, 3)
    fc, fc_disp = twin(ctx, pay, lens)
    for scale in (12000.0, 40000.0):
        disp, _ = check(ctx, pay, lens, fc, scale, n_fft)
        assert disp == fc_disp + "+k_sc16_narrow", disp


def test_laboratory_keys_select_the_two_pass_path_and_its_chunks(api):
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    p = payload_for(ctx, 16)
    pay, lens = payloads(ctx, 3500, 5, p), ragged(ctx, p)
    fc, fc_disp = twin(ctx, pay, lens)
    assert fc_disp == "k_txframe64"
    ctx.set_tuning("no_txframe64_sc16", 1)                       # the A/B key inside the fused envelope
    disp, _ = check(ctx, pay, lens, fc, 40000.0, "no_txframe64_sc16")
    assert disp == "k_txframe64+k_sc16_narrow", disp
    for chunk in (1, 2):                                         # chunk boundaries inside the batch: counts land at the right rows
        ctx.set_tuning("sc16_chunk_frames", chunk)
        disp, counts = check(ctx, pay, lens, fc, 40000.0, ("chunk", chunk))
        assert disp == "k_txframe64+k_sc16_narrow" and sum(counts) > 0, (disp, counts)
    ctx.set_tuning("sc16_chunk_frames", 0)
    ctx.set_tuning("no_txframe64_sc16", 0)
    disp, _ = check(ctx, pay, lens, fc, 40000.0, "fused again")
    assert disp == "k_txframe64_sc16"
    ctx.set_tuning("no_txframe64", 1)                            # the fc32 family's own key takes the fused sc16 kernel out too
    ctx.set_tuning("no_mid_kernels", 1)
    fc2, fc2_disp = twin(ctx, pay, lens)
    assert fc2_disp == "k_sym<tx>+k_tx_finish"
    disp, _ = check(ctx, pay, lens, fc2, 40000.0, "generic")
    assert disp == "k_sym<tx>+k_tx_finish+k_sc16_narrow", disp


# ------------------------------------------------------------------ 5. modes
@pytest.mark.parametrize("ecc", [1, 32, 80], ids=["hamming74", "rs255_k7f_r34", "ldpc648_fcs"])
def test_coded_modes_share_the_coding_layers(api, ecc):
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True, ecc=ecc)
    p = 100
    assert ctx.data_symbols(p) <= 56
    pay, lens = payloads(ctx, 3600 + ecc, 5, p), ragged(ctx, p)
    fc, fc_disp = twin(ctx, pay, lens)
    assert fc_disp.split("+")[-1] == "k_txframe64", fc_disp
    for scale in (12000.0, 40000.0):
        disp, _ = check(ctx, pay, lens, fc, scale, ecc)
        assert disp == fc_disp + "_sc16" and disp.split("+")[-1] == "k_txframe64_sc16", (disp, fc_disp)


# ------------------------------------------------------------------ 6. clipping on real frames
def test_clipped_counts_on_real_frames(api):
    """normalize divides by the signed maximum: BPSK without guard bands clips at full scale in every frame, 64-QAM with guard bands
    never does (tests/test_sc16_tx_cpu.py restates both on the oracle)."""
    import torch

    ctx = api.Context(n_fft=64, modulation=api.BPSK, guard_bands=False)
    pay = payloads(ctx, 3700, 8, 20)
    fc, _ = twin(ctx, pay)
    disp, counts = check(ctx, pay, None, fc, 32767.0, "bpsk")
    assert disp == "k_txframe64_sc16" and all(k >= 1 for k in counts), counts
    ctx = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True)
    pay = payloads(ctx, 3701, 8, 100)
    fc, _ = twin(ctx, pay)
    disp, counts = check(ctx, pay, None, fc, 32767.0, "qam64")
    assert counts == [0] * 8
    q = ctx.encode_batch_sc16(pay, 32767.0)                      # clipped_dev = NULL
    assert ctx.last_dispatch() == "k_txframe64_sc16"
    qn = q.cpu().numpy()
    assert np.array_equal(qn, narrowed(fc, 32767.0)[0]) and all(int(qn[f].max()) == 32767 for f in range(8))
    ctx.set_tuning("no_txframe64_sc16", 1)                       # ... and on the two-pass path
    assert torch.equal(ctx.encode_batch_sc16(pay, 32767.0), q) and ctx.last_dispatch() == "k_txframe64+k_sc16_narrow"


# ------------------------------------------------------------------ 7. the host path
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_encode_equals_the_device_call(api, pinned):
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    p = payload_for(ctx, 9)
    n, frame = 7, ctx.frame_samples(p)
    pay, lens = payloads(ctx, 3800, n, p), ragged(ctx, p, n)
    want, want_clipped = ctx.encode_batch_sc16(pay, 40000.0, lens=lens, want_clipped=True)
    want, want_clipped = want.cpu().numpy(), want_clipped.cpu().numpy()
    assert want_clipped.sum() > 0
    pay_h, lens_h = pay.cpu().numpy(), lens.cpu().numpy()
    for chunk in (1, 3, 0):
        for stride in (frame, frame + 3):
            out = api.pinned_empty((n, stride, 2), np.int16) if pinned else np.zeros((n, stride, 2), np.int16)
            out[:] = SENTINEL
            got, clipped = ctx.encode_host_sc16(pay_h, 40000.0, lens=lens_h, chunk_frames=chunk, out=out, want_clipped=True)
            assert np.array_equal(got[:, :frame], want) and np.array_equal(clipped, want_clipped), (chunk, stride)
            assert (got[:, frame:] == SENTINEL).all(), (chunk, stride)
        got = ctx.encode_host_sc16(pay_h, 40000.0, lens=lens_h, chunk_frames=chunk)          # clipped_host = NULL
        assert np.array_equal(got, want), chunk


# ------------------------------------------------------------------ 8. arguments
def test_argument_checks(api):
    import torch

    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    lib, h = ctx.lib, ctx.h
    p = 40
    frame = ctx.frame_samples(p)
    pay = torch.zeros((2, p), dtype=torch.uint8, device=ctx.device)
    out = torch.full((2, frame, 2), SENTINEL, dtype=torch.int16, device=ctx.device)
    enc = lambda *a: lib.ofdm_tx_encode_sc16_batch(h, *a)
    pay_h, out_h = np.zeros((2, p), np.uint8), np.full((2, frame, 2), SENTINEL, np.int16)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert enc(pay.data_ptr(), 2, p, None, p, bad, out.data_ptr(), frame, None) == -1
        assert lib.ofdm_tx_encode_sc16_host(h, pay_h.ctypes.data, 2, p, None, p, bad, out_h.ctypes.data, frame, None, 0) == -1
    assert lib.ofdm_tx_encode_sc16_host(h, pay_h.ctypes.data, 2, p, None, p, 1000.0, out_h.ctypes.data, frame - 1, None, 0) == -1
    assert lib.ofdm_tx_encode_sc16_host(h, pay_h.ctypes.data, 0, p, None, p, 1000.0, out_h.ctypes.data, frame, None, 0) == 0
    assert (out_h == SENTINEL).all()
    assert enc(pay.data_ptr(), 2, p, None, p, 1000.0, out.data_ptr(), frame - 1, None) == -1       # out_stride < frame
    assert enc(pay.data_ptr(), 2, p, None, p, 1000.0, None, frame, None) == -1                     # NULL out with frames
    assert enc(pay.data_ptr(), 2, p - 1, None, p, 1000.0, out.data_ptr(), frame, None) == -1       # payload_stride < payload_bytes, 2 frames
    assert enc(pay.data_ptr(), 0, p, None, p, 1000.0, out.data_ptr(), frame, None) == 0            # n_frames == 0
    assert enc(None, 0, p, None, p, 1000.0, None, frame, None) == 0
    ctx.synchronize()
    assert bool((out == SENTINEL).all())
    fcs = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True, ecc=api.ECC_FCS)
    big = 0x7FFFFFFF - 4                                                                           # payload_bytes + 8 > INT32_MAX
    assert fcs.lib.ofdm_tx_encode_sc16_batch(fcs.h, pay.data_ptr(), 1, big, None, big, 1000.0, out.data_ptr(), 1 << 40, None) == -2
    assert fcs.lib.ofdm_tx_encode_batch(fcs.h, pay.data_ptr(), 1, big, None, big, out.data_ptr(), 1 << 40) == -2     # as the twin
    q = torch.zeros((4000, 2), dtype=torch.int16, device=ctx.device)
    ob = torch.zeros((64,), dtype=torch.uint8, device=ctx.device)
    import ctypes as C
    ln, st = C.c_int32(), C.c_int32()
    for bad in (0.0, float("nan")):
        assert lib.ofdm_rx_decode_long_sc16(h, q.data_ptr(), 4000, bad, 0, 0, -1, 2, ob.data_ptr(), 64, C.byref(ln), C.byref(st), None, None, None) == -1
    assert lib.ofdm_rx_decode_long_sc16(h, q.data_ptr() + 2, 3000, 1.0, 0, 0, -1, 2, ob.data_ptr(), 64, C.byref(ln), C.byref(st), None, None, None) == -1


# ------------------------------------------------------------------ 9. round trip
def test_round_trip_through_sc16_on_both_sides(api):
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    p = 60
    pay = payloads(ctx, 3900, 4, p)
    q, clipped = ctx.encode_batch_sc16(pay, 12000.0, want_clipped=True)
    assert clipped.cpu().numpy().tolist() == [0] * 4            # 16-QAM with guard bands stays inside +-1.2: 12000 does not clip
    res = ctx.decode_batch_sc16(q, max_symbols=ctx.data_symbols(p), scale=1.0 / 12000.0)
    assert res["status"].cpu().numpy().tolist() == [0] * 4 and res["len"].cpu().numpy().tolist() == [p] * 4
    assert np.array_equal(res["bytes"].cpu().numpy()[:, :p], pay.cpu().numpy())
    data = bytes(np.random.default_rng(3901).integers(0, 256, 300, dtype=np.uint8))
    q = api.encode(data, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True, sc16_scale=32767.0)
    assert q.dtype == np.int16 and q.ndim == 2 and q.shape[1] == 2 and int(q.max()) == 32767
    tx = api.encode(data, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True)
    assert np.array_equal(q, sc16_ref.narrow(tx.astype(np.complex64), 32767.0)[0])
    assert api.decode(q, guard_bands=True, modulation=api.QAM64, ecc=api.ECC_LDPC648, fcs=True) == data


# ------------------------------------------------------------------ 10. one long capture
def long_capture(n_fft, mod, seed, **ctx_kw):
    """(context, payload, int16 capture [20000, 2] on the host, scale, D): one frame of tools/link.py's seeded link placed at sample 7 001
    of a 20 000-sample capture, quantised with its peak at 0.9 of full scale.  Instead of exact zeros the capture carries a seeded noise
    floor at 1e-3 of the frame's peak (about 30 LSB after quantisation): the Schmidl-Cox metric of an all-zero window is 0 / 0, and a
    detector that is compared bit for bit should be compared on numbers; the capture without a frame (q_empty) is that floor alone.  The
    N = 256 case uses QPSK."""
    c, pay, rx, D = _link(0, n_fft, mod, 1, 100, 25.0, seed, guard=True, **ctx_kw)
    rx = rx[0].cpu().numpy()
    rng = np.random.default_rng(seed)
    sigma = 1e-3 * float(np.abs(rx).max())
    cap = (sigma * (rng.standard_normal(20000) + 1j * rng.standard_normal(20000))).astype(np.complex64)
    empty = cap.copy()
    cap[7001: 7001 + rx.size] += rx
    q, scale = sc16_ref.quantise(cap, 0.9)
    q_empty, _ = sc16_ref.narrow(empty, np.float32(1.0) / scale)
    return c, pay[0].cpu().numpy(), q, q_empty, float(scale), D


def same_long(got, want, what):
    for k in ("status", "len", "offset"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("f_delta", "metric"):
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (what, k, got[k], want[k])
    gb, wb = got["bytes"], want["bytes"]
    gb = gb.cpu().numpy() if hasattr(gb, "cpu") else gb
    wb = wb.cpu().numpy() if hasattr(wb, "cpu") else wb
    assert bytes(gb[: want["len"]]) == bytes(wb[: want["len"]]), what


@pytest.mark.parametrize("n_fft,mod,ctx_kw", [(64, 4, {}), (256, 2, {"cfo_mode": 3})], ids=["n64", "n256_cfowide"])
def test_long_capture_equals_decode_long_on_the_widened_capture(api, n_fft, mod, ctx_kw):
    c, pay, q, q_empty, scale, D = long_capture(n_fft, mod, 4000 + n_fft, **ctx_kw)
    wide = c.to_device(sc16_ref.widen(q, scale))
    qd = c.to_device(q)
    want = c.decode_long(wide, D)
    fc_disp = c.last_dispatch()
    got = c.decode_long_sc16(qd, D, scale=scale)
    assert c.last_dispatch() == "k_sc16_widen+" + fc_disp, (c.last_dispatch(), fc_disp)
    same_long(got, want, "whole")
    assert want["status"] == 0 and want["len"] == 100 and bytes(want["bytes"].cpu().numpy()[:100]) == bytes(pay)
    assert abs(want["offset"] - 7001) < 200
    want_lo = c.decode_long(wide, D, lag_lo=3000)
    fc_disp = c.last_dispatch()
    same_long(c.decode_long_sc16(qd, D, scale=scale, lag_lo=3000), want_lo, "lag_lo")
    assert c.last_dispatch() == "k_sc16_widen+" + fc_disp and want_lo["status"] == 0
    d, _, _ = c.sc_correlate_long(wide)
    assert d > 6900
    want_k = c.decode_long(wide, D, d_hat_known=d)
    same_long(c.decode_long_sc16(qd, D, scale=scale, d_hat_known=d), want_k, "d_hat_known")
    assert want_k["status"] == 0
    # no frame: OFDM_FRAME_NOSYNC from both
    want_e = c.decode_long(c.to_device(sc16_ref.widen(q_empty, scale)), D)
    got_e = c.decode_long_sc16(c.to_device(q_empty), D, scale=scale)
    same_long(got_e, want_e, "empty")
    assert want_e["status"] == api.FRAME_NOSYNC
    # the host call, pageable and pinned, equals the device call
    same_long(c.decode_long_host_sc16(q, D, scale=scale), got, "host pageable")
    pin = api.pinned_empty(q.shape, np.int16)
    pin[:] = q
    same_long(c.decode_long_host_sc16(pin, D, scale=scale), got, "host pinned")
    assert c.last_dispatch().startswith("k_sc16_widen+")


def test_free_function_decode_long_takes_an_int16_capture(api):
    c, pay, q, _, scale, D = long_capture(64, 4, 4064)
    res = api.decode_long(q, guard_bands=True, modulation=api.QAM16, max_symbols=D, scale=scale)
    assert res["status"] == 0 and res["len"] == 100 and bytes(res["bytes"].cpu().numpy()[:100]) == bytes(pay)
