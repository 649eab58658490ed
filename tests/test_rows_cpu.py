"""The row-layout helper of tests/rows.py on numpy stand-ins, and the f64 definitions' indifference to what lies behind a row: no GPU."""
import numpy as np
import pytest

import rows as R
from gain_cases import cpu_case
from util import wide


@pytest.mark.parametrize("fill,dtype", [("u8", np.uint8), ("i8", np.int8), ("fc32", np.complex64), ("tone", np.complex64), (R.FILL_U8_OTHER, np.uint8)])
def test_embed_and_only_rows_written_round_trip(fill, dtype):
    rng = np.random.default_rng(1)
    for lay in R.output_layouts(40) + R.payload_layouts(37) + R.input_layouts(33):
        n = 3
        data = rng.integers(1, 100, (n, lay.row)).astype(dtype)
        flat, ptr = R.embed(None, data, lay, fill)
        assert flat.dtype == dtype and flat.size == lay.size(n) and flat.ctypes.data % 128 == 0
        assert ptr == flat.ctypes.data + lay.base_off * flat.dtype.itemsize
        assert np.array_equal(R.read_rows(flat, lay, n).view(np.uint8), data.view(np.uint8))
        assert R.only_rows_written(flat, lay, n, fill)
        blank, bptr = R.embed(None, None, lay, fill, n=n)
        assert bptr - blank.ctypes.data == ptr - flat.ctypes.data
        assert R.only_rows_written(blank, lay, n, fill, lens=[0] * n)       # nothing at all was written
        assert R.only_rows_written(flat, lay, n, fill, lens=[lay.row] * n)


def test_fills_are_the_stated_bit_patterns():
    assert R.host_bytes(R.fill_buffer("u8", 3)).tolist() == [0xEE] * 3
    assert R.fill_buffer("i8", 2).tolist() == [-128, -128]
    f = R.fill_buffer("fc32", 2)
    assert f.view(np.int32).tolist() == [0x7FC0DEAD, 0x7FC0BEEF] * 2 and np.isnan(f.real).all() and np.isnan(f.imag).all()
    t = R.fill_buffer("tone", 500)
    assert np.isfinite(t.view(np.float32)).all() and np.allclose(np.abs(t), 1e3, rtol=1e-6) and np.unique(t).size == 500
    assert (t.view(np.float32) != 0).all()


@pytest.mark.parametrize("fill", ["u8", "i8", "fc32", "tone"])
def test_a_one_byte_write_outside_the_rows_is_caught(fill):
    n = 3
    for lay in (R.Layout(16, 48 + 40, 40), R.Layout(3, 45, 40), R.Layout(1, 40, 40), R.Layout(0, 41, 40)):
        flat, _ = R.embed(None, None, lay, fill, n=n)
        item = flat.dtype.itemsize
        spots = [lay.start(n - 1) + lay.row,            # just behind the last row
                 lay.size(n) - 1]                       # the last element of the tail
        if lay.stride > lay.row:
            spots.append(lay.start(0) + lay.row)        # just behind row 0: the slack between rows
        if lay.base_off:
            spots.append(lay.base_off - 1)              # just before the base
        for e in spots:
            for byte in {0, item - 1}:
                b = flat.view(np.uint8)
                at = e * item + (byte if e != lay.base_off - 1 else item - 1 - byte)
                old = b[at]
                b[at] ^= 0x01
                assert not R.only_rows_written(flat, lay, n, fill), (lay, e, byte)
                b[at] = old
        assert R.only_rows_written(flat, lay, n, fill)
        b = flat.view(np.uint8)
        b[lay.start(1) * item] ^= 0x80                  # inside a row: allowed ...
        assert R.only_rows_written(flat, lay, n, fill)
        assert not R.only_rows_written(flat, lay, n, fill, lens=[lay.row, 0, lay.row])   # ... unless the row's own length forbids it


def test_the_layout_lists_hold_every_class_the_launchers_test():
    outs = [R.alignment_class(lay) for lay in R.output_layouts(2304)]
    assert {b for b, _ in outs} == {128, 16, 4, 1}
    assert {s for _, s in outs} == {"dense", 16, 4, 1}
    assert outs[0] == (128, "dense")
    # the same list over fc32 rows (transmit frames): 16-byte stores need base % 16 == 0 in BYTES and an even sample stride
    tx = [(lay.base_off * 8 % 16, lay.stride % 2) for lay in R.output_layouts(1120)]
    assert {(0, 0), (8, 0), (0, 1), (8, 1)} <= set(tx)
    ins = R.input_layouts(640)
    assert {lay.base_off * 8 % 16 for lay in ins} == {0, 8} and {lay.stride % 2 for lay in ins} == {0, 1}
    assert ins[0].dense() and all(lay.stride > lay.row for lay in ins[1:])
    pay = R.payload_layouts(300)
    assert {(lay.base_off | lay.stride) % 4 == 0 for lay in pay} == {True, False} and pay[0].dense()
    assert any(lay.base_off % 4 for lay in pay) and any(lay.stride % 4 and not lay.base_off for lay in pay)


def test_the_f64_normalize_ignores_what_lies_behind_the_row(orc):
    rng = np.random.default_rng(2)
    row = (rng.standard_normal(333) + 1j * rng.standard_normal(333)).astype(np.complex64)
    dense = orc.normalize(wide(row))
    for lay in R.input_layouts(row.size):
        flat, _ = R.embed(None, np.stack([row, row]), lay, "tone")
        for f in range(2):
            got = orc.normalize(wide(flat[lay.start(f): lay.start(f) + lay.row]))
            assert np.array_equal(got.view(np.uint64), dense.view(np.uint64))
    assert np.abs(flat).max() > 100 * np.abs(row).max()        # the slack would have moved the maximum


def test_the_f64_decode_reads_zeros_from_frame_len_on(orc):
    """samples at or beyond frame_len read as zero (pad_chunk, receiver.rs:203-210): the oracle's decode of the row cut at frame_len and
    of the row zeroed from frame_len on are the same decode, whatever the stride holds on the device"""
    case = cpu_case(64, 6, 100)
    rx = wide(case["rx"])
    for frame_len in (rx.size, rx.size - 160 - 40):              # the whole capture; half a symbol short of the frame's end
        cut = orc.decode_sc(rx[:frame_len], True, 6, 64, max_symbols=case["D"])
        padded = rx.copy()
        padded[frame_len:] = 0
        padded = np.concatenate([padded, np.zeros(77)])
        full = orc.decode_sc(padded, True, 6, 64, max_symbols=case["D"])
        assert cut["status"] == 0
        for k in ("status", "offset", "f_delta", "metric", "bytes", "n_symbols"):
            assert cut[k] == full[k], (frame_len, k)
