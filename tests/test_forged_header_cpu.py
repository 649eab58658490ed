"""CPU checks of tests/util.forge_frame (a frame whose 16-byte length header is forged) and of the oracle's reading of such headers:
the helper must reproduce orc.encode when the header is the honest one, and orc.decode_sc / orc.decode_given must follow the rule
of src/receiver.rs:85-95 for every forged value.  The GPU side (tests/test_gpu_forged_header.py) uses the same helper, the same
values and the oracle as its reference, so both are pinned here first."""
import numpy as np
import pytest

from util import forge_frame, header_bytes, header_values, rel_err, through_channel, wide

CONFIGS = [(64, 6, True, 560), (64, 1, True, 116), (256, 2, False, 300), (1024, 4, True, 900)]


def _shape(orc, n, mod, guard, nbytes):
    bps = orc.data_carriers(n, guard) * mod // 8
    D = -(-(16 + nbytes) // bps)
    return bps, D, D * bps - 16


@pytest.mark.parametrize("n,mod,guard,nbytes", CONFIGS)
def test_honest_header_reproduces_the_encoder(orc, n, mod, guard, nbytes):
    rng = np.random.default_rng(n + mod)
    for ln in (nbytes, nbytes - 1, 1, 0):
        pay = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        got = forge_frame(orc, header_bytes(ln, 0) + pay, n, guard, mod)
        want = orc.encode(pay, guard, mod, n)
        assert got.shape == want.shape
        assert rel_err(got, want) <= 1e-12, (ln, rel_err(got, want))


@pytest.mark.parametrize("n,mod,guard,nbytes", CONFIGS)
def test_oracle_follows_the_header_rule(orc, n, mod, guard, nbytes):
    rng = np.random.default_rng(7 * n + mod)
    S = n + n // 4
    bps, D, B = _shape(orc, n, mod, guard, nbytes)
    pairs = header_values(B)
    assert len(pairs) == 26
    for i, (lo, hi) in enumerate(pairs):
        body = bytes(rng.integers(0, 256, B, dtype=np.uint8))           # fills the D data symbols: the decoder sees B body bytes
        frame = forge_frame(orc, header_bytes(lo, hi) + body, n, guard, mod, allow_louder=mod == 1)
        assert frame.size == (10 + D) * S
        # the rule, in plain integers: the header is a little-endian u128; only a value below the body length shortens the body
        value = lo + (hi << 64)
        keep = value if value < B else B
        assert keep == (lo if (hi == 0 and lo < B) else B)
        given = orc.decode_given(frame, 0, 0.0, guard, mod, n, max_symbols=D)
        assert (given["status"], given["n_symbols"]) == (0, D), (lo, hi)
        assert given["bytes"] == body[:keep], (lo, hi, len(given["bytes"]), keep)
        # and through the whole receiver: delay, FIR channel, CFO, no noise
        cap = through_channel(orc, rng, frame, frame.size + S, 3 + i % 5, 0.3 * np.pi / S, snr_db=None, data_start=10 * S)
        sc = orc.decode_sc(wide(cap), guard, mod, n, max_symbols=D)
        assert sc["status"] == 0, (lo, hi)
        assert sc["bytes"] == body[:keep], (lo, hi, len(sc["bytes"]), keep)
        # one symbol fewer: the rule is applied to the body the decoder sees, not to the one that was sent
        if D > 1:
            B1 = (D - 1) * bps - 16
            cut = orc.decode_given(frame, 0, 0.0, guard, mod, n, max_symbols=D - 1)
            assert cut["bytes"] == body[:(value if value < B1 else B1)], (lo, hi)


def test_a_frame_louder_than_its_header_is_refused_unless_allowed(orc):
    """BPSK with guard bands: the 48 equal bits of a header of ones are a symbol of 48 equal points, 1.6 times the header's full scale.
    The helper refuses such a stream by default; with allow_louder the frame is the oracle's normalize of the splice -- the whole
    frame divided by its new maximum, the header blocks included."""
    n, mod, guard = 64, 1, True
    S, B = 80, 20 * 6 - 16
    body = bytes(np.random.default_rng(1).integers(0, 256, B, dtype=np.uint8))
    stream = header_bytes(2 ** 64 - 1, 0) + body
    with pytest.raises(AssertionError, match="louder"):
        forge_frame(orc, stream, n, guard, mod)
    loud = forge_frame(orc, stream, n, guard, mod, allow_louder=True)
    honest = orc.encode(body, guard, mod, n)
    peak = max(loud.real.max(), loud.imag.max())
    k = int(np.argmax(np.maximum(loud.real, loud.imag)))
    assert peak == 1.0 and 10 * S <= k < 11 * S                          # full scale is now in the first data symbol
    scale = loud[:10 * S].real.max()
    assert 0.55 < scale < 0.65                                           # 1 / 1.635
    assert rel_err(loud[:10 * S], scale * honest[:10 * S]) <= 1e-15
    assert rel_err(loud[12 * S:], scale * honest[12 * S:]) <= 1e-12      # symbols 0 and 1 hold the header, symbol 2 its last 4 bytes
