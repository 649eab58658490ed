"""Assertions the GPU tests of the frame modes share (tests/test_gpu_soft.py, _conv, _framed, _rs, _fcs, _ldpc, _chest): what every
mode must hold whatever its code is.  The links they run over are tools/link.py; what a chain must deliver is tests/chain_refs.py."""
import numpy as np
import torch

KEYS = ("status", "len", "offset", "f_delta", "metric")


def ofdm_api():
    """the library's Python face, imported on first use: collecting the tests needs no built library"""
    from ofdm_amd import api

    return api


def _host(b):
    return np.asarray(b.cpu() if torch.is_tensor(b) else b)


def assert_rows_are(r, want):
    """want: {frame: (status, out_len, bytes)}; bytes past out_len are not written and not compared"""
    status, ln, by = r["status"].cpu().numpy(), r["len"].cpu().numpy(), r["bytes"].cpu().numpy()
    for f, (st, n_out, data) in want.items():
        assert (int(status[f]), int(ln[f])) == (st, n_out), (f, status[f], ln[f], st, n_out)
        assert bytes(by[f, :n_out]) == bytes(data), f


def assert_same_rows(a, b):
    """two results (device or host) with the same KEYS and, per frame, the same out_len bytes"""
    for k in KEYS:
        if torch.is_tensor(a[k]) and torch.is_tensor(b[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            np.testing.assert_array_equal(_host(a[k]), _host(b[k]), err_msg=k)
    ba, bb = _host(a["bytes"]), _host(b["bytes"])
    for f, n_out in enumerate(_host(a["len"])):
        assert bytes(ba[f, :n_out]) == bytes(bb[f, :n_out]), f


def assert_entry_points_agree(api, c, rx, D, decode_kw=None, chunk_frames=2):
    """decode_batch against decode_host in chunks; then every frame alone: a one-row decode_batch against decode_long and
    decode_long_host, and, where its status is 0 and decode_kw (ecc = ..., fcs = ...) is given, against api.decode.
    -> (the batch result, [(status, out_len, offset, bytes) of every one-row decode])"""
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    assert_same_rows(r, c.decode_host(rx.cpu().numpy(), max_symbols=D, chunk_frames=chunk_frames))
    ones = []
    for f in range(rx.shape[0]):
        cap = rx[f].contiguous()
        one = c.decode_batch(cap.reshape(1, -1), max_symbols=D)
        st, n_out, off = int(one["status"][0]), int(one["len"][0]), int(one["offset"][0])
        data = bytes(one["bytes"][0, :n_out].cpu().numpy())
        for res in (c.decode_long(cap, D), c.decode_long_host(cap.cpu().numpy(), D)):
            assert (res["status"], res["len"], res["offset"]) == (st, n_out, off), f
            assert bytes(_host(res["bytes"])[:n_out]) == data, f
        if st == 0 and decode_kw is not None:
            assert api.decode(cap.cpu().numpy(), c.guard_bands, c.modulation, n_fft=c.n_fft, **decode_kw) == data, f
        ones.append((st, n_out, off, data))
    return r, ones


def assert_chunking_changes_nothing(c, rx, D, r):
    """the decode again in chunks of 3 frames of the LLR workspace (laboratory key soft_chunk_frames): the same rows -> that result"""
    c.set_tuning("soft_chunk_frames", 3)
    try:
        r3 = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
    finally:
        c.set_tuning("soft_chunk_frames", 0)
    assert_same_rows(r, r3)
    return r3


def assert_refuses_short_rows(c, rx, D, need, accepts=False):
    """ofdm_rx_decode_batch itself, frame 0 of rx: an output row one byte shorter than `need`, the most the chain can write, is
    refused (-1) before anything runs; accepts: a row of `need` bytes is taken -> [out_len, status] of the frame"""
    out = torch.zeros((1, max(need, 8)), dtype=torch.uint8, device=c.device)
    i32 = torch.zeros((2,), dtype=torch.int32, device=c.device)
    f = c.lib.ofdm_rx_decode_batch
    args = (c.h, rx.data_ptr(), 1, rx.shape[1], rx.shape[1], 0, D, out.data_ptr())
    tail = (i32.data_ptr(), i32[1:].data_ptr(), None, None, None)
    assert f(*args, need - 1, *tail) == -1
    if not accepts:
        return None
    assert f(*args, need, *tail) == 0
    c.synchronize()
    return i32.tolist()
