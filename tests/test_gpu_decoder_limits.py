"""GPU checks of the decoders where only their own construction tells the answer: the Viterbi kernels (k_viterbi_k7, k_viterbi_k7f) at
the longest row the entry points accept, 2^20 steps, and the finishing kernel of every coded frame mode (k_viterbi_k7, k_viterbi_k7f,
k_rs255_decode, k_ldpc_decode, k_rx_finish_soft) with short frames decoded behind long ones on the same wavefront.  No reference decoder is needed: a
code word at full confidence decodes to its own input, and a frame sent over a clean channel to its own payload.  Everything compared
here is bytes and integers; nothing has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
from chain_checks import assert_same_rows, ofdm_api as _api  # noqa: E402
from tools.link import generator, seeded_channel  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_STEPS = 1 << 20                                                     # kViterbiMaxSteps (ofdm_abi.hip)
PAYLOAD = (1 << 17) - 1                                                 # + the zero tail byte: 2^17 bytes = 2^20 steps


def _ctx(ecc, **kw):
    api = _api()
    return api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, ecc=ecc, **kw)


def _bits(coded: torch.Tensor) -> torch.Tensor:
    """[rows, n] bytes -> [rows, 8 n] bits, LSB first"""
    shifts = torch.arange(8, dtype=torch.uint8, device=coded.device)
    return ((coded[:, :, None] >> shifts) & 1).reshape(coded.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------- (a) the accepted maximum
# Every wavefront walks 2^20 dependent steps and a traceback of the same length.  Measured on an MI355X, one launch between the
# context's timer events (the tests print it): k_viterbi_k7, 3 rows of 2^20 steps, 66.5 ms terminated and 66.4 ms unterminated, 66.7 ms
# at 2^20 - 1 and 66.6 ms at 2^20 - 33 steps; k_viterbi_k7f, 1 row of 2^20 steps, 64.5 ms at rate 2/3 and 64.7 ms at rate 3/4.  The
# rows' wavefronts run side by side, so a launch costs what one row costs: about 63 ns a step.  The fixture (payloads, the encoder
# against the restatement on one row, the LLR rows) takes 0.7 s, each test 0.07 .. 0.13 s.
@pytest.fixture(scope="module")
def longest():
    api = _api()
    c = _ctx(api.ECC_CONV_K7)
    g = generator(c, 1 << 20)
    pay = torch.randint(0, 256, (3, PAYLOAD), dtype=torch.uint8, device=c.device, generator=g)
    coded = c.conv_encode(pay)
    c.synchronize()
    assert coded.shape == (3, 1 << 18)
    # the encoder at this length against the restatement: one row (a million Python steps)
    np.testing.assert_array_equal(coded[0].cpu().numpy(), cr.encode(pay[0].cpu().numpy().tobytes()))
    bits = _bits(coded).to(torch.int16)
    llr = torch.empty((3, 2 * MAX_STEPS), dtype=torch.int8, device=c.device)
    llr[0] = (bits[0] * 254 - 127).to(torch.int8)                       # +-127
    llr[1] = (bits[1] * 255 - 128).to(torch.int8)                       # 0 -> -128, 1 -> +127: the largest step the int32 metrics can see
    llr[2] = (bits[2] * 2 - 1).to(torch.int8)                           # +-1
    want = torch.cat([pay, torch.zeros((3, 1), dtype=torch.uint8, device=c.device)], dim=1)   # the payload, then the tail byte
    return c, pay, llr, want


def _timed(c, f):
    c.synchronize()
    c.timer_start()
    out = f()
    ms = c.timer_stop_ms()
    return out, ms


@pytest.mark.parametrize("terminated", [True, False])
def test_viterbi_at_the_accepted_maximum(longest, terminated):
    """3 rows of 2^20 steps: a full-confidence code word beats every other path by at least the free distance (the open end: by at
    least both coded bits of the last step), so the decode is the payload and its zero tail byte in both modes, at every LLR scale."""
    c, pay, llr, want = longest
    got, ms = _timed(c, lambda: c.viterbi_decode_soft(llr, n_steps=MAX_STEPS, terminated=terminated))
    c.synchronize()
    print(f"k_viterbi_k7, 3 rows of 2^20 steps, terminated={terminated}: {ms:.1f} ms")
    assert c.last_dispatch() == "k_viterbi_k7"
    assert got.shape == (3, MAX_STEPS // 8)
    for r in range(3):
        assert torch.equal(got[r], want[r]), (terminated, r, int((got[r] != want[r]).sum()))


@pytest.mark.parametrize("n_steps", [MAX_STEPS - 1, MAX_STEPS - 33])
def test_viterbi_just_below_the_maximum(longest, n_steps):
    """a ragged last 32-step block (2^20 - 1) and a ragged last 64-step fetch as well (2^20 - 33): the same LLR rows cut short,
    decoded unterminated"""
    c, pay, llr, want = longest
    got, ms = _timed(c, lambda: c.viterbi_decode_soft(llr, n_steps=n_steps, terminated=False))
    c.synchronize()
    print(f"k_viterbi_k7, 3 rows of {n_steps} steps: {ms:.1f} ms")
    n_out = n_steps // 8
    assert got.shape == (3, n_out)
    # the last byte is left out of the comparison: it lies next to the open end, where the cut decides, not the code word's margin
    for r in range(3):
        assert torch.equal(got[r, :n_out - 1], want[r, :n_out - 1]), (n_steps, r, int((got[r, :n_out - 1] != want[r, :n_out - 1]).sum()))


@pytest.mark.parametrize("rate", [1, 2])
def test_punctured_viterbi_at_the_accepted_maximum(longest, rate):
    """rates 2/3 and 3/4 through ofdm_conv_k7_encode_punctured / ofdm_conv_k7_decode_punctured: one row of 2^20 steps, +-127 at the
    kept positions"""
    c, pay, _, want = longest
    kept = int(c.lib.ofdm_conv_k7_kept_bits(MAX_STEPS, rate))
    coded = c.conv_encode(pay[:1], rate=rate)
    assert coded.shape == (1, (kept + 7) // 8)
    llr = (_bits(coded)[:, :kept].to(torch.int16) * 254 - 127).to(torch.int8).contiguous()
    for terminated in (True, False):
        got, ms = _timed(c, lambda: c.viterbi_decode_soft(llr, n_steps=MAX_STEPS, terminated=terminated, rate=rate))
        c.synchronize()
        print(f"k_viterbi_k7f, rate {rate}, 1 row of 2^20 steps, terminated={terminated}: {ms:.1f} ms")
        assert c.last_dispatch() == "k_viterbi_k7f"
        assert got.shape == (1, MAX_STEPS // 8)
        assert torch.equal(got[0], want[0]), (rate, terminated, int((got[0] != want[0]).sum()))


# ---------------------------------------------------------------------------------------------------------- (b) short behind long
P, FRAMES = 560, 24
LENGTHS = [P, 0, 1, P // 2, 17, P - 1]
# grid_cap 1 leaves one workgroup of four wavefronts: wavefront w decodes frames w, w + 4, ..., six frames of lengths
# LENGTHS[(w + 4 k) % 6] in turn -- 560, 17, 1, 560, 17, 1 on wavefront 0, 0, 559, 280, ... on wavefront 1 --, all into the one survivor
# slab, the one RS row state and the one LDPC pair walk it owns.
MODES = [  # (ecc, the kernel that finishes the frame, what is delivered)
    ("ECC_CONV_K7", "k_viterbi_k7", "exact"), ("ECC_CONV_K7F_R12", "k_viterbi_k7f", "exact"), ("ECC_CONV_K7F_R23", "k_viterbi_k7f", "exact"),
    ("ECC_CONV_K7F_R34", "k_viterbi_k7f", "exact"), ("ECC_RS255_K7F_R34", "k_rs255_decode", "rs"), ("ECC_RS255", "k_rs255_decode", "rs"),
    ("ECC_LDPC648", "k_ldpc_decode", "exact"), ("ECC_LDPC648_R56", "k_ldpc_decode<r56>", "exact"),
    ("ECC_HAMMING74_SOFT", "k_rx_finish_soft", "hamming"),
]


@pytest.mark.parametrize("name,kernel,delivers", MODES, ids=[m[0] for m in MODES])
def test_short_frames_behind_long_ones_on_one_wavefront(name, kernel, delivers):
    api = _api()
    c = _ctx(getattr(api, name))
    seed = 2400 + getattr(api, name)
    g = generator(c, seed)
    pay = torch.randint(0, 256, (FRAMES, P), dtype=torch.uint8, device=c.device, generator=g)
    lens = np.array([LENGTHS[f % len(LENGTHS)] for f in range(FRAMES)], np.int32)
    rx = seeded_channel(c, c.encode_batch(pay, lens=torch.from_numpy(lens)), 40.0, seed, g)
    D = c.data_symbols(P)
    base = c.decode_batch(rx, max_symbols=D)                            # the default grid: a wavefront a frame
    c.synchronize()
    c.set_tuning("grid_cap", 1)
    try:
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        trace = c.last_dispatch()
    finally:
        c.set_tuning("grid_cap", 0)
    assert kernel in trace.split("+"), trace
    status, ln, by = r["status"].cpu().numpy(), r["len"].cpu().numpy(), r["bytes"].cpu().numpy()
    host = pay.cpu().numpy()
    for f in range(FRAMES):
        p = int(lens[f])
        assert int(status[f]) == 0, (name, f, p, status.tolist())
        if delivers == "exact":
            assert int(ln[f]) == p, (name, f, p, ln.tolist())
        elif delivers == "rs":                                          # whole blocks, the always-present last one too; zeros behind the payload
            assert int(ln[f]) == 223 * (p // 223 + 2), (name, f, p, ln.tolist())
            assert not by[f, p:ln[f]].any(), (name, f, p)
        else:                                                           # whole 4-byte Hamming groups: up to 3 bytes of padding
            assert p <= int(ln[f]) <= p + 3, (name, f, p, ln.tolist())
        assert bytes(by[f, :p]) == bytes(host[f, :p]), (name, f, p)
    assert_same_rows(r, base)
