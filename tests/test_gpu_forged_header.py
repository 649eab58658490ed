"""Every device copy of the length-header rule (src/receiver.rs:85-95: keep = lo if (hi == 0 and lo < body) else body), fed headers
that no honest encoder writes: tests/util.forge_frame splices a forged 16-byte header (or, for the framed modes, a forged coded
length block) into an otherwise honest frame, tests/util.header_values lists the values -- small, odd, around the body length,
around 2^31, 2^32, 2^63 and 2^64, and with a high half that is not 0.  The references are the CPU oracle and the numpy
restatements, all pinned on the CPU (tests/test_forged_header_cpu.py, test_framed_cpu.py, test_conv_cpu.py, test_soft_cpu.py,
test_rs_modes_cpu.py).  Every test first shows that the forged bytes are what the device demodulated, names the kernel it reached,
and compares every frame: none is left out."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
import framed_ref as fr  # noqa: E402
import rs_vectors as rv  # noqa: E402
from chain_refs import UNCORRECTABLE, conv_reference_decode, hard_and_llrs, header_of, rs_composition, soft_reference_decode  # noqa: E402
from util import decision_margin, forge_frame, header_bytes, header_rule, header_values, through_channel, wide  # noqa: E402

pytestmark = pytest.mark.gpu

SNR_DB = 45.0        # on the data symbols: the uncoded header must arrive as forged (the FIR channel's weakest bins sit 10 dB lower)
TOL = 1e-5           # the suite's bar for f32 kernels against the f64 oracle: a hard decision may differ only this close to a boundary
RS_EXTRA = (254, 255, 256, 509, 510, 511, 764)   # a three-block code word is 765 bytes: every block whole, cut by one byte, or absent
_CACHE = {}


def _api():
    from ofdm_amd import api

    return api


def _ctx(fb, ecc=0, **tuning):
    return _api().Context(n_fft=fb.n, modulation=fb.mod, guard_bands=fb.guard, ecc=ecc, tuning=tuning or None)


# ---------------------------------------------------------------------------------------------------------- captures
def _body(kind, rng, B, i):
    if kind == "random":             # plain and Hamming modes: in Hamming mode arbitrary 7-bit words, double and triple errors included
        return bytes(rng.integers(0, 256, B, dtype=np.uint8))
    if kind == "conv":               # the convolutional code of a random payload ...
        assert B % 2 == 0 and B > 24
        if i % 3 == 0 and i < 26:    # ... whole: 2 (p + 1) = B bytes, the trellis ends in state 0
            return bytes(cr.encode(bytes(rng.integers(0, 256, B // 2 - 1, dtype=np.uint8))))
        # ... or cut, with 12 bytes that are no code behind it: whether the traceback starts in state 0 then changes delivered bytes
        code = cr.encode(bytes(rng.integers(0, 256, B // 2 + 10, dtype=np.uint8)))[:B - 12]
        return bytes(code) + bytes(rng.integers(0, 256, 12, dtype=np.uint8))
    if kind == "rs":                 # the three code words of a random payload: clean, 3 errors a block, or 20 errors in block 1
        code = np.frombuffer(_api().create_transmission_bytes(bytes(rng.integers(0, 256, 500, dtype=np.uint8))), np.uint8).copy()
        assert code.size == 765 <= B
        for blk, n_err in {0: (), 1: ((0, 3), (1, 3), (2, 3)), 2: ((1, 20),)}[i % 3]:
            pos = 255 * blk + rng.choice(255, n_err, replace=False)
            code[pos] ^= rng.integers(1, 256, n_err, dtype=np.uint8)
        return bytes(code) + bytes(rng.integers(0, 256, B - 765, dtype=np.uint8))
    raise ValueError(kind)


def _through(orc, rng, frame, S, i, snr_db=SNR_DB):
    """a delay of a few samples (both parities), a small CFO of either sign, the FIR channel, high SNR"""
    return through_channel(orc, rng, frame, frame.size + S + 48, 2 + (5 * i) % 23, 0.4 * ((i % 7) - 3) / 3 * np.pi / S, snr_db, data_start=10 * S)


def _forged(orc, n, mod, guard, D, kind="random", extra_lo=()):
    """one capture per forged header for a decoder that sees D data symbols; built once per configuration and shared"""
    key = (n, mod, guard, D, kind, extra_lo)
    if key not in _CACHE:
        bps = orc.data_carriers(n, guard) * mod // 8
        B, S = D * bps - 16, n + n // 4
        if kind == "conv":           # three more frames with lo = B, the one value at which `terminated` hangs on <= against <
            extra_lo = (B, B, B)
        pairs = header_values(B, extra_lo)
        assert len(pairs) == 26 + len(extra_lo)
        rng = np.random.default_rng([n, mod, D, len(kind)])
        caps, bodies = [], []
        for i, (lo, hi) in enumerate(pairs):
            body = _body(kind, rng, B, i)
            assert len(body) == B
            frame = forge_frame(orc, header_bytes(lo, hi) + body, n, guard, mod, allow_louder=mod == 1)
            assert frame.size == (10 + D) * S
            caps.append(_through(orc, rng, frame, S, i))
            bodies.append(body)
        _CACHE[key] = SimpleNamespace(n=n, mod=mod, guard=guard, D=D, B=B, S=S, bps=bps, pairs=pairs, bodies=bodies, caps=np.stack(caps), oracle=None)
    return _CACHE[key]


def _oracle(orc, fb):
    if fb.oracle is None:
        fb.oracle = [orc.decode_sc(wide(c), fb.guard, fb.mod, fb.n, max_symbols=fb.D, want_soft=True) for c in fb.caps]
    return fb.oracle


# ---------------------------------------------------------------------------------------------------------- running and comparing
def _host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _decode(c, fb):
    rx = c.to_device(fb.caps)
    r = c.decode_batch(rx, max_symbols=fb.D)
    c.synchronize()
    return rx, r, c.last_dispatch()


def _decode_abi(c, rx, D, pad=0, misalign=0):
    """ofdm_rx_decode_batch through the C ABI: rows of decode_row_bytes(D) + pad bytes in a buffer of 0xEE with one spare row behind
    the last, the first row `misalign` bytes off a dword.  -> (result as decode_batch returns it, the buffer as rows [F + 1, stride])"""
    F, row = rx.shape[0], c.decode_row_bytes(D)
    stride = row + pad
    buf = torch.full(((F + 1) * stride + 8,), 0xEE, dtype=torch.uint8, device=c.device)
    assert buf.data_ptr() % 4 == 0
    r = {"len": c.empty((F,), torch.int32), "status": c.empty((F,), torch.int32), "offset": c.empty((F,), torch.int32),
         "f_delta": c.empty((F,), torch.float64), "metric": c.empty((F,), torch.float32)}
    rc = c.lib.ofdm_rx_decode_batch(c.h, rx.data_ptr(), F, rx.shape[1], rx.shape[1], 0, D, buf.data_ptr() + misalign, stride, r["len"].data_ptr(),
                                    r["status"].data_ptr(), r["offset"].data_ptr(), r["f_delta"].data_ptr(), r["metric"].data_ptr())
    assert rc == 0, rc
    c.synchronize()
    rows = buf[misalign:misalign + (F + 1) * stride].view(F + 1, stride)
    r["bytes"] = rows[:F, :row]
    return r, rows


def _assert_headers_arrived(c, rx, r, fb):
    """the 16 hard bytes the device demodulates with the chain's own offset / f_delta / channel estimate are the forged ones"""
    hard, _ = hard_and_llrs(c, rx, r, fb.D, want_llr=False)
    got = [header_of(row) for row in hard]
    assert got == fb.pairs, [(f, got[f], fb.pairs[f]) for f in range(len(got)) if got[f] != fb.pairs[f]]


def _on_a_boundary(got, want, soft, mod):
    """the suite's rule for hard decisions (tests/test_gpu_parity.py): body bit b is stream bit 128 + b, point (128 + b) // mod"""
    if len(got) != len(want):
        return False
    g = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
    w = np.unpackbits(np.frombuffer(want, np.uint8), bitorder="little")
    pts = np.unique((128 + np.nonzero(g != w)[0]) // mod)
    return bool(np.all(decision_margin(np.asarray(soft)[pts], mod) < TOL))


def _assert_is_oracle(orc, fb, r, hamming, what):
    """status, offset, CFO, length and bytes of every frame against orc.decode_sc on the same capture (then orc.hamming74_decode)"""
    r = _host(r)
    bad = []
    for f, (lo, hi) in enumerate(fb.pairs):
        w = _oracle(orc, fb)[f]
        assert w["status"] == 0 and len(w["bytes"]) == header_rule(lo, hi, fb.B), (f, lo, hi)    # the oracle read the forged header too
        want = orc.hamming74_decode(w["bytes"])[0] if hamming else w["bytes"]
        n_out = int(r["len"][f])
        got = bytes(r["bytes"][f, :max(n_out, 0)])
        if (int(r["status"][f]), int(r["offset"][f]), n_out) != (0, w["offset"], len(want)) or abs(r["f_delta"][f] - w["f_delta"]) > 1e-9:
            bad.append((f, hex(lo), hex(hi), int(r["status"][f]), int(r["offset"][f]), n_out, w["offset"], len(want)))
        elif got != want and (hamming or not _on_a_boundary(got, want, w["soft"], fb.mod)):
            bad.append((f, hex(lo), hex(hi), "bytes"))
    assert not bad, (what, bad)


def _assert_is_reference(fb, r, want, what):
    """(out_len, bytes) per frame, every frame with status 0"""
    r = _host(r)
    assert len(want) == len(fb.pairs) and (r["status"] == 0).all(), (what, r["status"].tolist())
    bad = [(f, hex(fb.pairs[f][0]), hex(fb.pairs[f][1]), int(r["len"][f]), n_out) for f, (n_out, data) in want.items()
           if int(r["len"][f]) != n_out or bytes(r["bytes"][f, :n_out]) != data]
    assert not bad, (what, bad)


def _names(dispatch):
    return dispatch.split("+")


# ---------------------------------------------------------------------------------------------------------- 1. ECC_NONE, N = 64
def test_rxframe64_fused_finish(orc):
    fb = _forged(orc, 64, 6, True, 6)
    assert fb.B % 4 == 0                                     # decode_batch's own rows are dword rows: the kernel finishes the frame itself
    for tuning in ({}, {"no_rxframe64_split": 1}, {"grid_cap": 1}):
        c = _ctx(fb, 0, **tuning)
        rx, r, disp = _decode(c, fb)
        _assert_headers_arrived(c, rx, r, fb)
        assert "k_rxframe64<finish>" in _names(disp) and "k_rx_finish" not in _names(disp), disp
        assert ("k_rxframe64<cut,list>" in _names(disp)) == ("no_rxframe64_split" not in tuning), disp
        _assert_is_oracle(orc, fb, r, False, tuning)


def test_rxframe64_then_k_rx_finish_for_rows_off_a_dword(orc):
    fb = _forged(orc, 64, 6, True, 6)
    c = _ctx(fb, 0)
    rx = c.to_device(fb.caps)
    r, rows = _decode_abi(c, rx, fb.D, misalign=1)
    disp = c.last_dispatch()
    _assert_headers_arrived(c, rx, r, fb)
    assert rows.data_ptr() % 4 == 1
    assert "k_rxframe64" in _names(disp) and "k_rx_finish" in _names(disp) and "k_rxframe64<finish>" not in _names(disp), disp
    _assert_is_oracle(orc, fb, r, False, "out off a dword")
    assert bool((rows[-1] == 0xEE).all())


# ---------------------------------------------------------------------------------------------------------- 2. N = 1024 and N = 256
@pytest.mark.parametrize("hamming", [0, 1])
def test_rxframe1024_fused_finish_and_its_two_fallbacks(orc, hamming):
    fb = _forged(orc, 1024, 4, True, 3)
    for tuning, fused, frame_kernel in (({}, True, True), ({"no_rx1024_finish": 1}, False, True), ({"no_rxframe1024": 1}, False, False)):
        c = _ctx(fb, hamming, **tuning)
        rx, r, disp = _decode(c, fb)
        _assert_headers_arrived(c, rx, r, fb)
        assert ("k_rxframe1024<finish>" in _names(disp)) == fused and ("k_rx_finish" in _names(disp)) == (not fused), disp
        assert ("k_rxframe1024" in _names(disp)) == (frame_kernel and not fused), disp
        _assert_is_oracle(orc, fb, r, bool(hamming), tuning)


@pytest.mark.parametrize("hamming", [0, 1])
def test_generic_chain_and_k_rx_finish_at_n256(orc, hamming):
    fb = _forged(orc, 256, 2, False, 5)
    c = _ctx(fb, hamming)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    assert "k_rx_finish" in _names(disp) and "rxframe" not in disp, disp
    _assert_is_oracle(orc, fb, r, bool(hamming), "n256")


def test_hamming_bpsk_six_byte_symbols(orc):
    """the reference's default frame: BPSK with guard bands, 6 bytes a symbol.  A header of ones is a symbol of 48 equal points, louder
    than the frame's header blocks: forge_frame(allow_louder) normalises such a frame as the encoder would have"""
    fb = _forged(orc, 64, 1, True, 8)
    assert fb.bps == 6 and fb.B == 32
    c = _ctx(fb, 1)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    assert "k_rxframe64" in _names(disp) and "k_rx_finish" in _names(disp), disp
    _assert_is_oracle(orc, fb, r, True, "bpsk")


# ---------------------------------------------------------------------------------------------------------- 3. soft Hamming
@pytest.mark.parametrize("n,mod,D", [(64, 6, 6), (1024, 4, 3)])
def test_k_rx_finish_soft(orc, n, mod, D):
    api = _api()
    fb = _forged(orc, n, mod, True, D)
    c = _ctx(fb, api.ECC_HAMMING74_SOFT)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    assert "k_rx_finish_soft" in _names(disp), disp
    want = soft_reference_decode(c, rx, r, fb.D)
    assert [want[f][0] for f in range(len(fb.pairs))] == [header_rule(lo, hi, fb.B) // 7 * 4 for lo, hi in fb.pairs]
    _assert_is_reference(fb, r, want, "soft")
    c3 = _ctx(fb, api.ECC_HAMMING74_SOFT, soft_chunk_frames=3)   # many chunks of the LLR workspace
    _, r3, disp3 = _decode(c3, fb)
    assert "k_rx_finish_soft" in _names(disp3), disp3
    _assert_is_reference(fb, r3, want, "soft, chunks of 3")


# ---------------------------------------------------------------------------------------------------------- 4. CONV_K7
@pytest.mark.parametrize("n,mod,D", [(64, 6, 6), (1024, 4, 3)])
def test_k_viterbi_k7_chain_mode(orc, n, mod, D):
    api = _api()
    fb = _forged(orc, n, mod, True, D, kind="conv")
    c = _ctx(fb, api.ECC_CONV_K7)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    assert "k_viterbi_k7" in _names(disp), disp
    want = conv_reference_decode(c, rx, r, fb.D)
    # T = 4 keep and the clamp of n_out, spelled out: keep 0 .. 3 deliver nothing, an odd keep rounds down
    assert [want[f][0] for f in range(len(fb.pairs))] == [max(header_rule(lo, hi, fb.B) // 2 - 1, 0) for lo, hi in fb.pairs]
    assert [want[f][0] for f in range(10)] == [0, 0, 0, 0, 1, 2, 2, 3, 5, 6]
    # lo = B (frame 13 and the three extra frames) is decoded terminated, lo = B + 1 (frame 14) and every invalid header unterminated;
    # on these bodies -- a cut code word with 12 random bytes behind it -- that changes delivered bytes: the reference of a lo = B
    # frame is not what the other traceback gives
    _, L = hard_and_llrs(c, rx, r, fb.D)
    assert fb.pairs[13] == (fb.B, 0) and fb.pairs[14] == (fb.B + 1, 0) and fb.pairs[26:] == [(fb.B, 0)] * 3
    n_out = fb.B // 2 - 1
    differ = 0
    for f, terminated in ((13, True), (14, False), (26, True), (27, True), (28, True)):
        both = [bytes(cr.viterbi(L[f, 128:128 + 8 * fb.B], terminated=t)[:n_out]) for t in (terminated, not terminated)]
        assert want[f] == (n_out, both[0]), f
        differ += terminated and both[0] != both[1]
    assert differ >= 1
    _assert_is_reference(fb, r, want, "conv")
    for tuning in ({"soft_chunk_frames": 3}, {"grid_cap": 1}):
        c2 = _ctx(fb, api.ECC_CONV_K7, **tuning)
        _, r2, disp2 = _decode(c2, fb)
        assert "k_viterbi_k7" in _names(disp2), disp2
        _assert_is_reference(fb, r2, want, tuning)


# ---------------------------------------------------------------------------------------------------------- 5. RS255 around ECC_NONE
def test_rs_outer_code_takes_its_code_len_from_the_header(orc):
    api = _api()
    fb = _forged(orc, 64, 6, True, 22, kind="rs", extra_lo=RS_EXTRA)     # 22 symbols: the smallest body that holds three RS blocks
    assert fb.B >= 765 and RS_EXTRA[-1] == 765 - 1
    c = _ctx(fb, api.ECC_RS255)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    assert "k_rxframe64<finish>" in _names(disp) and "k_rs255_decode" in _names(disp), disp
    ri, want = rs_composition(c, rx, fb.D)
    # what the inner mode hands over as code_len is the rule's value (the inner mode itself is held to the oracle above)
    assert ri["len"].tolist() == [header_rule(lo, hi, fb.B) for lo, hi in fb.pairs] and (ri["status"] == 0).all()
    rh = _host(r)
    bad = [(f, hex(fb.pairs[f][0]), int(rh["status"][f]), int(rh["len"][f]), st, n_out) for f, (st, n_out, data) in enumerate(want)
           if (int(rh["status"][f]), int(rh["len"][f])) != (st, n_out) or bytes(rh["bytes"][f, :n_out]) != data]
    assert not bad, bad
    for k in ("offset", "f_delta", "metric"):
        assert torch.equal(r[k], ri[k]), k
    # rows of every outcome: nothing to correct, corrected, uncorrectable
    ib, il = ri["bytes"].cpu().numpy(), ri["len"].cpu().numpy()
    seen = set()
    for f, (st, n_out, data) in enumerate(want):
        fixed = rv.host_row(c.lib, ib[f], int(il[f]))[2]
        assert (fixed < 0) == (st == UNCORRECTABLE), f
        seen.add("uncorrectable" if fixed < 0 else "fixed" if fixed else "clean")
    assert seen == {"clean", "fixed", "uncorrectable"}, seen


# ---------------------------------------------------------------------------------------------------------- 6. entry points
@pytest.mark.parametrize("kind", ["random", "conv"])
def test_host_and_long_entry_points_read_the_same_header(orc, kind):
    api = _api()
    fb = _forged(orc, 64, 6, True, 6, kind=kind)
    c = _ctx(fb, api.ECC_CONV_K7 if kind == "conv" else api.ECC_NONE)
    rx, r, _ = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)
    rh = _host(r)
    assert (rh["status"] == 0).all()
    host = c.decode_host(fb.caps, max_symbols=fb.D, chunk_frames=2)
    bad = []
    for f in range(len(fb.pairs)):
        n_out = int(rh["len"][f])
        want = (0, n_out, bytes(rh["bytes"][f, :n_out]))
        lg = c.decode_long(rx[f].contiguous(), fb.D)
        for name, got in (("host", (int(host["status"][f]), int(host["len"][f]), bytes(host["bytes"][f, :n_out]))),
                          ("long", (lg["status"], lg["len"], bytes(lg["bytes"][:n_out].cpu().numpy())))):
            if got != want:
                bad.append((name, f, hex(fb.pairs[f][0]), hex(fb.pairs[f][1]), got[:2], want[:2]))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- 7. framed modes
FRAMED_P = 100          # payload bytes really there: 7, 6 and 5 data symbols at rates 1/2, 2/3 and 3/4


def _framed_shape(orc, rate):
    bps = orc.data_carriers(64, True) * 6 // 8
    D = -(-(16 + fr.coded_len(FRAMED_P, rate)) // bps)
    return SimpleNamespace(n=64, mod=6, guard=True, D=D, B=D * bps - 16, S=80, bps=bps)


def _framed_caps(orc, fb, streams, seed):
    rng = np.random.default_rng(seed)
    caps = []
    for i, (head, stream) in enumerate(streams):
        pad = bytes(rng.integers(0, 256, fb.B - len(stream), dtype=np.uint8))
        caps.append(_through(orc, rng, forge_frame(orc, head + stream + pad, 64, True, 6, allow_louder=True), fb.S, i))
    return np.stack(caps)


def _framed_reference(c, rx, r, fb, rate):
    _, L = hard_and_llrs(c, rx, r, fb.D)
    return [fr.decode_stream(L[f, 128:128 + 8 * fb.B], fb.B, rate) for f in range(rx.shape[0])]


@pytest.mark.parametrize("rate", [0, 1, 2])
def test_framed_modes_ignore_the_legacy_header(orc, rate):
    api = _api()
    key = ("framed-a", rate)
    if key not in _CACHE:
        fb = _framed_shape(orc, rate)
        fb.pairs = header_values(fb.B)
        fb.payload = bytes(np.random.default_rng(50 + rate).integers(0, 256, FRAMED_P, dtype=np.uint8))
        stream = bytes(fr.encode_stream(fb.payload, rate))
        fb.caps = _framed_caps(orc, fb, [(header_bytes(lo, hi), stream) for lo, hi in fb.pairs], 60 + rate)
        _CACHE[key] = fb
    fb = _CACHE[key]
    c = _ctx(fb, api.ECC_CONV_K7F_R12 + rate)
    rx, r, disp = _decode(c, fb)
    _assert_headers_arrived(c, rx, r, fb)                     # the 26 legacy headers did arrive: they are ignored, not missing
    assert "k_viterbi_k7f" in _names(disp), disp
    rh = _host(r)
    want = _framed_reference(c, rx, r, fb, rate)
    assert want == [(0, fb.payload)] * 26                     # identical for all 26, and the payload
    got = [(int(rh["status"][f]), bytes(rh["bytes"][f, :max(int(rh["len"][f]), 0)])) for f in range(26)]
    assert got == want, [(f, hex(fb.pairs[f][0]), hex(fb.pairs[f][1]), got[f][0], len(got[f][1])) for f in range(26) if got[f] != want[f]]


def _framed_lengths(fb, rate):
    avail = fb.B - fr.LENGTH_BLOCK
    fits = max(p for p in range(avail + 1) if fr.body_len(p, rate) <= avail)
    assert fr.body_len(fits + 1, rate) > avail and fits > FRAMED_P + 1
    return [0, 1, FRAMED_P, FRAMED_P + 1, fits, fits + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]


def _framed_b(orc, rate):
    key = ("framed-b", rate)
    if key not in _CACHE:
        fb = _framed_shape(orc, rate)
        fb.lengths = _framed_lengths(fb, rate)
        payload = bytes(np.random.default_rng(70 + rate).integers(0, 256, FRAMED_P, dtype=np.uint8))
        body = bytes(fr.encode_punctured(payload, rate))
        honest = header_bytes(fr.coded_len(FRAMED_P, rate), 0)
        fb.blocks = [bytes(fr.length_block(p)) for p in fb.lengths]
        fb.caps = _framed_caps(orc, fb, [(honest, blk + body) for blk in fb.blocks], 80 + rate)
        _CACHE[key] = fb
    return _CACHE[key]


@pytest.mark.parametrize("rate", [0, 1, 2])
def test_framed_modes_take_any_valid_length_block(orc, rate):
    """length blocks with a correct complement and tail in front of a body that really holds FRAMED_P bytes, declaring less, more, the
    most that fits, one more than fits, and lengths around 2^31 and 2^32"""
    api = _api()
    fb = _framed_b(orc, rate)
    c = _ctx(fb, api.ECC_CONV_K7F_R12 + rate)
    rx, r, disp = _decode(c, fb)
    hard, _ = hard_and_llrs(c, rx, r, fb.D, want_llr=False)
    assert [bytes(row[16:16 + fr.LENGTH_BLOCK]) for row in hard] == fb.blocks     # the forged length blocks arrived intact
    assert "k_viterbi_k7f" in _names(disp), disp
    rh = _host(r)
    want = _framed_reference(c, rx, r, fb, rate)
    avail = fb.B - fr.LENGTH_BLOCK
    cut = fr.max_steps(8 * avail, rate) // 8                  # what a body that does not fit delivers at most
    assert [(st, len(data)) for st, data in want] == [(0, p if fr.body_len(p, rate) <= avail else min(p, cut)) for p in fb.lengths]
    got = [(int(rh["status"][f]), int(rh["len"][f])) for f in range(len(want))]
    assert got == [(st, len(data)) for st, data in want], (fb.lengths, got)
    bad = [hex(fb.lengths[f]) for f, (st, data) in enumerate(want) if bytes(rh["bytes"][f, :len(data)]) != data]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- 8. nothing outside the row
def _any_caps(orc, ecc):
    api = _api()
    if ecc in (api.ECC_CONV_K7F_R12, api.ECC_CONV_K7F_R23, api.ECC_CONV_K7F_R34, api.ECC_RS255_K7F_R12, api.ECC_RS255_K7F_R23, api.ECC_RS255_K7F_R34):
        return _framed_b(orc, ecc % 10)
    if ecc == api.ECC_RS255:
        return _forged(orc, 64, 6, True, 22, kind="rs", extra_lo=RS_EXTRA)
    if ecc == api.ECC_HAMMING74:
        return _forged(orc, 1024, 4, True, 3)
    return _forged(orc, 64, 6, True, 6, kind="conv" if ecc == api.ECC_CONV_K7 else "random")


@pytest.mark.parametrize("ecc", [0, 1, 2, 5, 10, 11, 12, 20, 30, 31, 32])
def test_no_write_outside_the_row(orc, ecc):
    fb = _any_caps(orc, ecc)
    c = _ctx(fb, ecc)
    rx = c.to_device(fb.caps)
    row = c.decode_row_bytes(fb.D)
    r, rows = _decode_abi(c, rx, fb.D, pad=32)
    if hasattr(fb, "pairs"):
        _assert_headers_arrived(c, rx, r, fb)
    else:
        hard, _ = hard_and_llrs(c, rx, r, fb.D, want_llr=False)
        assert [bytes(h[16:16 + fr.LENGTH_BLOCK]) for h in hard] == fb.blocks
    assert rows.shape == (rx.shape[0] + 1, row + 32)
    assert bool((rows[:-1, row:] == 0xEE).all()), "bytes behind a row were written"
    assert bool((rows[-1] == 0xEE).all()), "the spare row was written"
    ln = r["len"].cpu().numpy()
    assert ((0 <= ln) & (ln <= row)).all(), ln.tolist()
