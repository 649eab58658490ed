"""Row layouts for the batch entry points of include/ofdm_hip.h (tests/test_rows_cpu.py, tests/test_gpu_rows.py).

Every batch call takes its rows as (base, stride, length).  A Layout places n rows of `row` elements at base_off + f * stride of one
flat buffer whose first element is 128-byte aligned; embed() builds that buffer with a fill everywhere else, only_rows_written()
requires the fill to be there still, byte for byte.  The fills are fixed bit patterns and never zeros: an output fill no kernel
produces (0xEE bytes; a NaN pair with a payload for fc32; -128 for LLRs), an input slack that is LOUD and finite -- a tone of amplitude
1e3 behind fc32 rows (a NaN in the slack would prove nothing about a maximum), 0xEE behind payload rows.

The ctypes callers at the end go to ctx.lib with the signatures of ofdm_amd/_lib.py and take explicit strides; they return the status
instead of raising, so that a refusal can be asserted.  Nothing here touches a GPU at import."""
import ctypes as C
from typing import NamedTuple

import numpy as np

TAIL = 64                       # elements kept (and checked) behind the last row
FILL_U8 = 0xEE
FILL_U8_OTHER = 0x11            # the second payload slack of the transmit tests
FILL_I8 = -128
FILL_FC32 = (0x7FC0DEAD, 0x7FC0BEEF)   # int32 pair: (re, im) of a quiet NaN with a payload
TONE_AMPLITUDE = 1e3
TONE_STEP = 0.37                # rad / sample


class Layout(NamedTuple):
    """n rows of `row` elements: row f at elements [base_off + f * stride, + row) of the flat buffer"""
    base_off: int
    stride: int
    row: int

    def start(self, f):
        return self.base_off + f * self.stride

    def size(self, n):
        """elements of the flat buffer: everything up to the end of row n - 1 and TAIL elements more"""
        return self.base_off + max(n - 1, 0) * self.stride + self.row + TAIL

    def dense(self):
        return self.base_off == 0 and self.stride == self.row


def fill_buffer(fill, count):
    """count elements of a fill: "u8" (0xEE), an int (that byte), "i8" (-128), "fc32" (the NaN pair), "tone" (loud, finite, every sample
    different so that a row read one sample off changes the answer)"""
    if fill == "u8":
        return np.full(count, FILL_U8, np.uint8)
    if isinstance(fill, (int, np.integer)):
        return np.full(count, int(fill), np.uint8)
    if fill == "i8":
        return np.full(count, FILL_I8, np.int8)
    if fill == "fc32":
        return np.tile(np.array(FILL_FC32, np.int32), count).view(np.complex64)
    if fill == "tone":
        t = TONE_AMPLITUDE * np.exp(1j * (TONE_STEP * np.arange(count, dtype=np.float64) + 0.5))
        return t.astype(np.complex64)
    raise ValueError(fill)


def output_layouts(r):
    """the (base offset, stride) forms every output is put through, over the dense row r: 128-aligned dense; 16-multiples with slack;
    4-multiples; odd"""
    return [Layout(0, r, r), Layout(0, r + 16, r), Layout(16, r + 48, r), Layout(0, r + 4, r), Layout(4, r + 4, r),
            Layout(0, r + 1, r), Layout(1, r, r), Layout(3, r + 5, r)]


def input_layouts(ln):
    """fc32 input rows: dense; base at 8 modulo 16 with an odd or even sample stride"""
    return [Layout(0, ln, ln), Layout(1, ln + 1, ln), Layout(0, ln + 7, ln)]


def payload_layouts(p):
    return [Layout(0, p, p), Layout(0, p + 3, p), Layout(1, p + 4, p), Layout(0, p + 64, p)]


def alignment_class(layout, itemsize=1):
    """(base class, stride class) in bytes: 128 / 16 / 4 / 1 for the base, "dense" / 16 / 4 / 1 for the stride"""
    def cls(v, top):
        for a in top:
            if v % a == 0:
                return a
        return 1
    b = cls(layout.base_off * itemsize, (128, 16, 4))
    s = "dense" if layout.stride == layout.row else cls(layout.stride * itemsize, (16, 4))
    return b, s


def _is_torch(a):
    return hasattr(a, "data_ptr")


def host_bytes(flat):
    """a flat buffer (numpy or torch, any dtype) as uint8 on the host"""
    a = flat.detach().cpu().numpy() if _is_torch(flat) else np.asarray(flat)
    if a.dtype.kind == "c":
        a = np.ascontiguousarray(a).view(np.float32)
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def embed(ctx, rows, layout, fill, n=None):
    """-> (flat, pointer to row 0).  flat holds `fill` everywhere and rows[f] at layout.start(f); rows = None: n blank rows (an output).
    ctx = None builds a numpy stand-in, otherwise a device tensor on the context's device (uploaded as raw bytes: the NaN fill keeps
    its payload).  The first element of flat is 128-byte aligned."""
    n = len(rows) if rows is not None else n
    host = fill_buffer(fill, layout.size(n))
    if rows is not None:
        rows = np.asarray(rows)
        assert rows.shape == (n, layout.row) and rows.dtype == host.dtype, (rows.shape, rows.dtype, host.dtype)
        assert n < 2 or layout.stride >= layout.row
        for f in range(n):
            host[layout.start(f): layout.start(f) + layout.row] = rows[f]
    item = host.dtype.itemsize
    if ctx is None:
        raw = np.empty(host.nbytes + 128, np.uint8)
        skip = (-raw.ctypes.data) % 128
        flat = raw[skip: skip + host.nbytes].view(host.dtype)
        flat[:] = host
        base = flat.ctypes.data
    else:
        import torch

        flat = torch.from_numpy(host.view(np.uint8)).to(ctx.device).view(torch.from_numpy(host[:1]).dtype)
        base = flat.data_ptr()
    assert base % 128 == 0, base
    return flat, base + layout.base_off * item


def read_rows(flat, layout, n):
    """the n rows of a flat buffer, on the host: [n, row]"""
    a = flat.detach().cpu().numpy() if _is_torch(flat) else np.asarray(flat)
    return np.stack([a[layout.start(f): layout.start(f) + layout.row] for f in range(n)])


def only_rows_written(flat, layout, n, fill, lens=None):
    """True iff every element outside the n row extents still holds `fill`, compared as raw bytes: the slack between rows, the part
    before the base and the TAIL behind the last row.  lens (optional): row f may only have changed in its first lens[f] elements."""
    got = host_bytes(flat)
    want = host_bytes(fill_buffer(fill, layout.size(n)))
    assert got.size == want.size, (got.size, want.size)
    item = want.size // layout.size(n)
    free = np.ones(got.size, bool)
    for f in range(n):
        ln = layout.row if lens is None else int(lens[f])
        free[layout.start(f) * item: (layout.start(f) + ln) * item] = False
    return bool(np.array_equal(got[free], want[free]))


# ---------------------------------------------------------------------------------------------------------------- ctypes callers
def _p(x):
    """None, an address, a torch tensor or a numpy array -> c_void_p"""
    if x is None:
        return None
    if _is_torch(x):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    return C.c_void_p(int(x))


def rx_demod(ctx, in_dev, n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, out_dev, out_stride, offset=None,
             f_delta=None, hk=None, hk_stride=0, soft=None):
    return ctx.lib.ofdm_rx_demod_batch(ctx.h, _p(in_dev), n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, _p(offset),
                                       _p(f_delta), _p(hk), hk_stride, _p(out_dev), out_stride, _p(soft))


def tx_encode(ctx, payload_dev, n_frames, payload_stride, payload_len, payload_bytes, out_dev, out_stride):
    return ctx.lib.ofdm_tx_encode_batch(ctx.h, _p(payload_dev), n_frames, payload_stride, _p(payload_len), payload_bytes, _p(out_dev),
                                        out_stride)


def rx_decode(ctx, in_dev, n_frames, frame_stride, frame_len, n_lags, max_symbols, out_dev, out_stride, out_len, status, offset=None,
              f_delta=None, metric=None):
    return ctx.lib.ofdm_rx_decode_batch(ctx.h, _p(in_dev), n_frames, frame_stride, frame_len, n_lags, max_symbols, _p(out_dev), out_stride,
                                        _p(out_len), _p(status), _p(offset), _p(f_delta), _p(metric))


def estimate_channel(ctx, in_dev, n_frames, frame_stride, frame_len, offset, f_delta, hk_dev):
    return ctx.lib.ofdm_estimate_channel_batch(ctx.h, _p(in_dev), n_frames, frame_stride, frame_len, _p(offset), _p(f_delta), _p(hk_dev))


def normalize(ctx, x_dev, n_frames, frame_stride, frame_len):
    return ctx.lib.ofdm_normalize_batch(ctx.h, _p(x_dev), n_frames, frame_stride, frame_len)


def cfo_rotate(ctx, x_dev, n_frames, frame_stride, frame_len, f_delta, first_index=None):
    return ctx.lib.ofdm_cfo_rotate_batch(ctx.h, _p(x_dev), n_frames, frame_stride, frame_len, _p(f_delta), _p(first_index))


def xcorr(ctx, a_dev, n_frames, a_stride, a_len, b_dev, nb, idx_max, peak=None, out_dev=None, out_stride=0):
    return ctx.lib.ofdm_xcorr_batch(ctx.h, _p(a_dev), n_frames, a_stride, a_len, _p(b_dev), nb, _p(idx_max), _p(peak), _p(out_dev), out_stride)


def frequency_correction(ctx, in_dev, n_pairs, stride, right_offset, f_delta):
    return ctx.lib.ofdm_frequency_correction_batch(ctx.h, _p(in_dev), n_pairs, stride, right_offset, _p(f_delta))


def rx_decode_host(ctx, in_host, n_frames, frame_stride, frame_len, n_lags, max_symbols, out_host, out_stride, out_len, status,
                   offset=None, f_delta=None, metric=None, chunk_frames=0):
    return ctx.lib.ofdm_rx_decode_host(ctx.h, _p(in_host), n_frames, frame_stride, frame_len, n_lags, max_symbols, _p(out_host), out_stride,
                                       _p(out_len), _p(status), _p(offset), _p(f_delta), _p(metric), chunk_frames)


def rx_demod_host(ctx, in_host, n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, out_host, out_stride, chunk_frames=0):
    return ctx.lib.ofdm_rx_demod_host(ctx.h, _p(in_host), n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, _p(out_host),
                                      out_stride, chunk_frames)
