#!/usr/bin/env python3
"""What ofdm_last_dispatch reports for a fixed list of calls, as JSON {case: dispatch string}.  Needs a GPU.

    python tools/dispatch_table.py [--commit HASH] [--out FILE]

The list covers every entry point whose string is put together from more than one launch site: the decode chains (hard, soft in two
chunks, outer-coded, combined), the sc16 entry points in two chunks of different size, the host pipe in two unequal chunks, the long
capture calls, the scan, the packets with one row a chunk, a channel-estimate smoothing over two chunks, and one empty call per family
behind a non-empty one.  tests/test_gpu_dispatch_table.py holds the strings to tests/golden/dispatch_parent.json, which is this tool's
output on the commit named in it: a change of the host layer that is meant to leave every string alone is measured against that file.
Only calls of ofdm_amd.api that the recorded commit has may be used here, so that the tool runs on both trees.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAMES, CHUNK = 6, 4   # two chunks of different size wherever a chunk is set
PAYLOAD = 200          # N = 64, 16-QAM, guard bands: 9 data symbols uncoded
CODED = 120            # ... and 10 to 15 under the coded modes
PAYLOAD_256 = 1000     # N = 256: 11 data symbols
SCALE = 1.0 / 8192.0


def table():
    import numpy as np
    import torch

    from ofdm_amd import api
    from tools.link import branch_link_on, link_on

    out = {}

    def note(name, c):
        assert name not in out, name
        out[name] = c.last_dispatch()

    def ctx(n=64, ecc=api.ECC_NONE, **kw):
        return api.Context(n_fft=n, modulation=api.QAM16, guard_bands=True, ecc=ecc, **kw)

    def host(t):
        return t.cpu().numpy()

    # ---- decode_batch: hard, soft in two chunks, outer-coded; the empty call
    for name, n, ecc, payload, kw in (
            ("n64_hard", 64, api.ECC_NONE, PAYLOAD, {}), ("n256_hard", 256, api.ECC_NONE, PAYLOAD_256, {}),
            ("n64_hamming", 64, api.ECC_HAMMING74, CODED, {}), ("n64_wls", 64, api.ECC_NONE, PAYLOAD, {"chest_mode": api.CHEST_WLS}),
            ("n64_soft_hamming", 64, api.ECC_HAMMING74_SOFT, CODED, {}), ("n64_conv_k7", 64, api.ECC_CONV_K7, CODED, {}),
            ("n64_k7f_r23_noise_weight", 64, api.ECC_CONV_K7F_R23, CODED, {"llr_weight": api.LLRW_NOISE}),
            ("n64_ldpc", 64, api.ECC_LDPC648, CODED, {}), ("n64_rs", 64, api.ECC_RS255, CODED, {}),
            ("n64_rs_k7f_r12", 64, api.ECC_RS255_K7F_R12, CODED, {}), ("n64_fcs_rs", 64, api.ECC_FCS + api.ECC_RS255, CODED, {}),
            ("n64_fcs_ldpc_r34", 64, api.ECC_FCS + api.ECC_LDPC648_R34, CODED, {}), ("n256_fcs_soft_hamming", 256, api.ECC_FCS + api.ECC_HAMMING74_SOFT, PAYLOAD_256 // 2, {})):
        c = ctx(n, ecc, **kw)
        c.set_tuning("soft_chunk_frames", CHUNK)
        _, rx = link_on(c, FRAMES, payload, 30.0, 11)
        D = c.data_symbols(payload)
        c.decode_batch(rx, D)
        note(f"decode_batch/{name}", c)
        c.decode_batch(rx[:0], D)
        note(f"decode_batch/{name}/empty", c)
        c.synchronize()

    # ---- decode_combine: three frames of two captures, two frames a chunk
    for name, ecc in (("k7f_r12", api.ECC_CONV_K7F_R12), ("fcs_ldpc", api.ECC_FCS + api.ECC_LDPC648)):
        c = ctx(64, ecc)
        c.set_tuning("soft_chunk_frames", 2)
        _, rx = branch_link_on(c, 3, CODED, [25.0, 22.0], 12)
        D = c.data_symbols(CODED)
        c.decode_combine(rx, D)
        note(f"decode_combine/{name}", c)
        c.decode_combine(rx[:0], D)
        note(f"decode_combine/{name}/empty", c)
        c.synchronize()

    # ---- the sc16 entry points, device and host, and the host pipe of the fc32 ones
    for n, payload in ((64, PAYLOAD), (256, PAYLOAD_256)):
        for fused in ((True, False) if n == 64 else (False,)):
            c = ctx(n)
            tag = f"n{n}" + ("" if n != 64 else "_fused" if fused else "_widened")
            c.set_tuning("sc16_chunk_frames", CHUNK)
            if n == 64 and not fused:
                c.set_tuning("no_demod64_sc16", 1)
                c.set_tuning("no_txframe64_sc16", 1)
            pay, rx = link_on(c, FRAMES, payload, 30.0, 13)
            D = c.data_symbols(payload)
            q, _ = c.sc16_narrow(rx, 1.0 / SCALE)
            c.decode_batch_sc16(q, D, scale=SCALE)
            note(f"decode_batch_sc16/{tag}", c)
            c.decode_batch_sc16(q[:0], D, scale=SCALE)
            note(f"decode_batch_sc16/{tag}/empty", c)
            sym = c.encode_batch(pay)[:, 10 * c.S:18 * c.S].contiguous()   # a regular stream of 8 symbols a row: the fused kernels' unit
            qs, _ = c.sc16_narrow(sym, 1.0 / SCALE)
            c.rx_demod_sc16(qs, 8, scale=SCALE)
            note(f"rx_demod_sc16/{tag}", c)
            c.rx_demod_sc16(qs[:0], 8, scale=SCALE)
            note(f"rx_demod_sc16/{tag}/empty", c)
            c.encode_batch_sc16(pay, 1.0 / SCALE, want_clipped=True)
            note(f"encode_batch_sc16/{tag}", c)
            c.encode_batch_sc16(pay[:0], 1.0 / SCALE)
            note(f"encode_batch_sc16/{tag}/empty", c)
            c.synchronize()
            c.decode_host_sc16(host(q), D, chunk_frames=CHUNK, scale=SCALE)
            note(f"decode_host_sc16/{tag}", c)
            c.demod_host_sc16(host(qs), 8, chunk_frames=CHUNK, scale=SCALE)
            note(f"demod_host_sc16/{tag}", c)
            c.encode_host_sc16(host(pay), 1.0 / SCALE, chunk_frames=CHUNK, want_clipped=True)
            note(f"encode_host_sc16/{tag}", c)
            if fused or n != 64:
                c.decode_host(host(rx), D, chunk_frames=CHUNK)
                note(f"decode_host/n{n}", c)
                c.decode_host(host(rx)[:0], D, chunk_frames=CHUNK)
                note(f"decode_host/n{n}/empty", c)
                c.demod_host(host(sym), 8, chunk_frames=CHUNK)
                note(f"demod_host/n{n}", c)
                c.demod_host(host(sym)[:0], 8, chunk_frames=CHUNK)
                note(f"demod_host/n{n}/empty", c)
                c.encode_host(host(pay), chunk_frames=CHUNK)
                note(f"encode_host/n{n}", c)
                c.encode_host(host(pay)[:0], chunk_frames=CHUNK)
                note(f"encode_host/n{n}/empty", c)

    # ---- one long capture: FRAMES packets back to back, each behind its delay and in front of noise
    for n, ecc, payload in ((64, api.ECC_NONE, PAYLOAD), (256, api.ECC_NONE, PAYLOAD_256), (64, api.ECC_FCS + api.ECC_CONV_K7F_R12, CODED)):
        c = ctx(n, ecc)
        tag = f"n{n}" + ("_fcs_k7f_r12" if ecc else "")
        _, rx = link_on(c, FRAMES, payload, 30.0, 14)
        D = c.data_symbols(payload)
        span = rx.shape[1]
        x = rx.reshape(-1).contiguous()
        c.decode_long(x, D)
        note(f"decode_long/{tag}/lag_lo_0", c)
        c.decode_long(x, D, lag_lo=span)
        note(f"decode_long/{tag}/lag_lo_{span}", c)
        c.decode_long(x, D, d_hat_known=c.sc_correlate_long(x)[0])
        note(f"decode_long/{tag}/d_hat_known", c)
        c.decode_long(x[:span].contiguous(), D)
        note(f"decode_long/{tag}/one_frame", c)
        c.sc_correlate_long(x, lag_lo=span)
        note(f"sc_correlate_long/{tag}", c)
        c.decode_long_host(host(x), D)
        note(f"decode_long_host/{tag}", c)
        q, _ = c.sc16_narrow(x, 1.0 / SCALE)
        c.decode_long_sc16(q, D, scale=SCALE)
        note(f"decode_long_sc16/{tag}/lag_lo_0", c)
        c.decode_long_sc16(q, D, scale=SCALE, lag_lo=span)
        note(f"decode_long_sc16/{tag}/lag_lo_{span}", c)
        c.decode_long_host_sc16(host(q), D, scale=SCALE)
        note(f"decode_long_host_sc16/{tag}", c)
        # every packet: the scan, the batched decode with one row a chunk (with and without the offsets), the host form
        hold = c.default_holdoff()
        det = c.sc_scan_long(x, hold, 16)
        note(f"sc_scan_long/{tag}", c)
        out[f"sc_scan_long/{tag}/detections"] = str(int(det["d_hat"].size))
        c.sc_scan_long(x[:0], hold, 16)
        note(f"sc_scan_long/{tag}/empty", c)
        c.sc_scan_long_host(host(x), hold, 16)
        note(f"sc_scan_long_host/{tag}", c)
        c.set_tuning("packets_chunk_rows", 1)
        c.decode_packets(x, det, D)
        note(f"decode_packets/{tag}/offsets", c)
        nd, ob = int(det["d_hat"].size), c.decode_row_bytes(D)
        by, ln, st = c.empty((max(nd, 1), ob), torch.uint8), c.empty((max(nd, 1),), torch.int32), c.empty((max(nd, 1),), torch.int32)
        dh, fd, m = (np.ascontiguousarray(det[k], dtype=t) for k, t in (("d_hat", np.int64), ("f_delta", np.float64), ("metric", np.float32)))
        c._ck(c.lib.ofdm_rx_decode_packets(c.h, api._dev(x), x.numel(), nd, api._host(dh), api._host(fd), api._host(m), D, api._dev(by), ob,
                                           api._dev(ln), api._dev(st), None, None, None), "rx_decode_packets")
        note(f"decode_packets/{tag}/no_offsets", c)
        c.decode_packets(x, {k: np.asarray(det[k])[:0] for k in ("d_hat", "f_delta", "metric")}, D)
        note(f"decode_packets/{tag}/empty", c)
        c.decode_all_host(host(x), hold, 16, D)
        note(f"decode_all_host/{tag}", c)
        c.set_tuning("packets_chunk_rows", 0)
        c.decode_all_host(host(x), hold, 16, D)
        note(f"decode_all_host/{tag}/one_chunk", c)
        c.synchronize()

    # ---- chest_smooth: 64 MiB of rows a chunk, so two chunks at N = 64 are 131072 rows and a few more
    c = ctx(64)
    hk = torch.zeros((131072 + 5, 64), dtype=torch.complex64, device=c.device)
    hk[:, 0] = 1.0
    c.chest_smooth(hk, out=hk)
    note("chest_smooth/n64_two_chunks", c)
    c.chest_smooth(hk[:0])
    note("chest_smooth/n64_two_chunks/empty", c)
    c.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", default="", help="recorded under \"commit\": the revision the library was built from")
    ap.add_argument("--out", help="write the JSON here as well")
    a = ap.parse_args()
    text = json.dumps({"commit": a.commit, "cases": table()}, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".tmp", "w") as f:
            f.write(text + "\n")
        os.replace(a.out + ".tmp", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
