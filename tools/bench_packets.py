#!/usr/bin/env python3
"""EXT-13 measurements: every packet of a long capture through ONE run of the receive chain (ofdm_rx_decode_packets) against the two
ways that decode one packet per call, one process on one MI355X -> profiles/packets_speed.json.

The captures are tools/bench_scan.py's: `--samples` samples (2 000 000) cut from the rows of tools/link.py's seeded link laid back to
back, 64-QAM with guard bands at 30 dB; N = 64 (29 data symbols: 3120-sample frames, about 600 of them) and N = 1024 (4 data symbols:
17 920-sample frames, about 110).

Per block, alternated in this one process, `--reps` passes each after one warm-up, wall clock (every way ends synchronised, with the
per-packet scalars on the host and the bytes on the device), median and spread (max - min):

  loop      decode_long(lag_lo = end of the last packet) until nothing is found (tests/test_gpu_host_path.py's loop)
  scan_loop one sc_scan_long, then decode_long(lag_lo = where the search for packet k started) per detection (api.decode_all())
  batched   one sc_scan_long, then ONE decode_packets (api.decode_all(batched=True))

Asserted in the same run: the three deliver the same packets -- status, length, offset and bytes equal, f_delta within 1e-9 and metric
within 1e-6.  Also: k_pkt_rows + k_gather_rows alone (laboratory key packets_gather_only; the context's event timer) next to
ofdm_hbm_read_probe (unit-stride 16-byte loads) over as many bytes as the gather reads; the gather writes as many again.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ofdm_amd import api  # noqa: E402
from tools.bench_scan import stat, wall_alternated  # noqa: E402
from tools.link import alternated_ms, link, open_record  # noqa: E402


def block(n_fft, data_symbols, samples, reps, seed):
    probe = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    payload = data_symbols * probe.bytes_per_symbol - 16
    frame = probe.frame_samples(payload)
    rows = samples // (frame + 160) + 1
    c, pay, rx, D = link(api.ECC_NONE, n_fft, api.QAM64, rows, payload, 30.0, seed)
    assert D == data_symbols and rx.shape[1] == frame + 160
    x = rx.reshape(-1)[:samples].contiguous()
    W = c.params.sync_window_reps * c.S
    holdoff = frame - W
    out = {}

    def loop():
        got, lo = [], 0
        while True:
            r = c.decode_long(x, D, lag_lo=lo)
            if r["status"] == api.FRAME_NOSYNC:
                break
            got.append(r)
            lo = max(lo + 1, r["offset"] + frame)
        out["loop"] = got

    def scan_loop():
        det = c.sc_scan_long(x, holdoff, 1 << 16)
        out["scan_loop"] = [c.decode_long(x, D, lag_lo=int(lo)) for lo in det["lag_lo"]]

    def batched():
        det = c.sc_scan_long(x, holdoff, 1 << 16)
        r = c.decode_packets(x, det, D)
        c.synchronize()
        out["batched"] = {k: (v if k == "bytes" else v.cpu().numpy()) for k, v in r.items()}

    ms = wall_alternated({"loop": loop, "scan_loop": scan_loop, "batched": batched}, reps)
    dispatch = c.last_dispatch()
    a, s, b = out["loop"], out["scan_loop"], out["batched"]
    n = len(a)
    assert len(s) == n and b["status"].size == n, (n, len(s), b["status"].size)

    def same(p, k):
        return all(p[f] == int(b[f][k]) for f in ("len", "status", "offset")) and abs(p["f_delta"] - float(b["f_delta"][k])) <= 1e-9 and \
            abs(p["metric"] - float(b["metric"][k])) <= 1e-6 and torch.equal(p["bytes"][: p["len"]], b["bytes"][k, : p["len"]])

    bad = [k for k in range(n) if not (same(a[k], k) and same(s[k], k))]
    assert not bad, f"the batched decode and the loops delivered different packets: {bad[:8]}"
    sent = sum(int(b["status"][k] == 0 and b["len"][k] == payload and torch.equal(b["bytes"][k, :payload], pay[k])) for k in range(n))
    R = min((10 + D) * c.S + 2, (samples + 1) & ~1)
    rec = {"n_fft": n_fft, "samples": samples, "frame_samples": frame, "data_symbols": data_symbols, "payload_bytes": payload, "packets": n,
           "payloads_delivered_exactly": sent, "holdoff": holdoff, "row_samples": R, "batched_dispatch": dispatch, "outputs_equal": True,
           "loop_of_decode_long": stat(ms["loop"]), "scan_then_decode_long": stat(ms["scan_loop"]), "scan_then_decode_packets": stat(ms["batched"])}
    bm = rec["scan_then_decode_packets"]["ms_median"]
    rec["ratio_loop_over_batched"] = round(rec["loop_of_decode_long"]["ms_median"] / bm, 2)
    rec["ratio_scan_loop_over_batched"] = round(rec["scan_then_decode_long"]["ms_median"] / bm, 2)

    det = c.sc_scan_long(x, holdoff, 1 << 16)
    probe_samples = min(n * R, samples) // 80 * 80
    c.set_tuning("packets_gather_only", 1)
    g = alternated_ms({"gather": (c, lambda: c.decode_packets(x, det, D)), "hbm_read_probe": (c, lambda: c.hbm_read_probe(x[:probe_samples], 2)),
                       "scan": (c, lambda: c.sc_scan_long(x, holdoff, 1 << 16))}, reps)
    c.set_tuning("packets_gather_only", 0)
    gm, pm = stat(g["gather"]), stat(g["hbm_read_probe"])
    rec["gather"] = {"bytes_read": 8 * n * R, "bytes_written": 8 * n * R,
                     "k_pkt_rows+k_gather_rows": {**gm, "read_gbytes_per_s": round(8 * n * R / gm["ms_median"] / 1e6, 2),
                                                  "note": "the event timer brackets the upload of the three detection arrays too"},
                     "hbm_read_probe": {**pm, "bytes": 8 * probe_samples, "read_gbytes_per_s": round(8 * probe_samples / pm["ms_median"] / 1e6, 2)},
                     "ratio_gather_over_probe": round(gm["ms_median"] / pm["ms_median"], 2)}
    rec["sc_scan_long_alone"] = stat(g["scan"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="n64,n1024")
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packets_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_packets.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process; one warm-up of every way, then alternated passes; wall clock (the gather, the read probe and the scan "
                     "alone: the context's event timer); median and spread (max - min)"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    for name, n_fft, syms, seed in (("n64", 64, 29, 1201), ("n1024", 1024, 4, 1202)):
        if name in a.blocks.split(","):
            rec[name] = block(n_fft, syms, a.samples, a.reps, seed)
            save()
            torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
