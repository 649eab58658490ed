"""The modes as a whole: every one of the 30 ecc values composes its lengths and its row size from its layers (tests/chain_refs.py:
mode_coded_len, mode_row_bytes over framed_ref, ldpc_ref and fcs_ref), and a context that encodes and decodes in turn keeps the
buffers of the two apart.  The files of the modes pin the same rules one mode at a time; only
test_encode_and_decode_take_turns_on_one_context launches a kernel.  The last test holds the list of modes itself to the library."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_refs import ALL_MODES, mode_coded_len, mode_row_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
FCS = 64
N_FFT, S, CARRIERS = 64, 80, 48              # guard bands on


@functools.lru_cache(maxsize=None)
def _ctx(ecc, modulation):
    from ofdm_amd import api

    return api.Context(n_fft=N_FFT, modulation=modulation, guard_bands=True, ecc=ecc)


@pytest.mark.parametrize("ecc", ALL_MODES)
def test_every_mode_composes_its_lengths(ecc):
    bps = 2                                  # QPSK
    c = _ctx(ecc, bps)
    assert (c.S, c.data_carriers) == (S, CARRIERS)
    for p in (0, 1, 39, 40, 222, 223, 224, 560):
        coded = mode_coded_len(ecc, p)
        points = -(-(16 + coded) * 8 // bps)
        nsym = -(-points // CARRIERS)
        assert (c.coded_len(p), c.data_symbols(p), c.frame_samples(p)) == (coded, nsym, (10 + nsym) * S), p


@pytest.mark.parametrize("ecc", ALL_MODES)
def test_every_mode_sizes_its_rows(ecc):
    """ofdm_rx_decode_batch with n_frames = 0: the row-size check comes before the early return"""
    c = _ctx(ecc, 2)

    def call(max_symbols, out_stride):
        return c.lib.ofdm_rx_decode_batch(c.h, None, 0, 4096, 4096, 0, max_symbols, None, out_stride, None, None, None, None, None)

    for max_symbols in (1, 3, 12):
        row = mode_row_bytes(ecc, max(max_symbols * c.bytes_per_symbol - 16, 0))
        assert call(max_symbols, row) == OK, (max_symbols, row)
        if row > 0:
            assert call(max_symbols, row - 1) == INVALID, (max_symbols, row)


@pytest.mark.parametrize("ecc", [0, 20, FCS + 32], ids=["no_outer_layer", "rs", "fcs_rs_k7f_r34"])
def test_encode_and_decode_take_turns_on_one_context(ecc):
    """encode -> decode -> encode -> decode on the same context, one mode per count of outer layers: the smallest shape at which two
    buffer roles in one workspace slot, or a layer peeled in the wrong order, shows"""
    c = _ctx(ecc, 1)                         # BPSK
    g = torch.Generator().manual_seed(ecc + 1)
    pay = torch.randint(0, 256, (3, 40), dtype=torch.uint8, generator=g).to(c.device)
    D = c.data_symbols(40)
    # bare RS delivers whole blocks, the payload zero-padded and the trailing zero block included; the frame check brings the length back
    want_len = 223 * (255 * (40 // 223 + 1) // 255 + 1) if ecc == 20 else 40
    seen = []
    for _ in range(2):
        tx = c.encode_batch(pay)
        rx = c.channel_batch(tx, snr_db=300.0, seed=5)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        seen.append(c.last_dispatch())
        assert r["status"].tolist() == [0, 0, 0] and r["len"].tolist() == [want_len] * 3
        assert torch.equal(r["bytes"][:, :40], pay) and not bool(r["bytes"][:, 40:want_len].any())
    assert seen[0] == seen[1] and seen[0]


def test_the_library_takes_exactly_the_listed_modes():
    """ALL_MODES is the library's own list: ofdm_create takes an ecc of 0 .. 127 exactly when the list has it, so a mode added to the
    library without the list (and with it without the chain tests that run over the list) turns this red"""
    from ofdm_amd import api

    taken = []
    for ecc in range(0, 128):
        if ecc in ALL_MODES:
            api.Context(n_fft=N_FFT, modulation=2, guard_bands=True, ecc=ecc).close()
            taken.append(ecc)
        else:
            with pytest.raises(api.OfdmError):
                api.Context(n_fft=N_FFT, modulation=2, guard_bands=True, ecc=ecc)
    assert sorted(taken) == sorted(ALL_MODES) and len(taken) == 30
