#!/usr/bin/env python3
"""EXT-12 measurements: finding every packet of a long capture in one pass (ofdm_sc_scan_long) against the loop a caller writes without
it, one process on one MI355X -> profiles/scan_speed.json.

The capture: `--samples` samples (2 000 000) cut from the rows of tools/link.py's seeded link laid back to back -- 64-QAM with guard
bands at 30 dB, every row one frame at a delay of 1 .. 32 samples with its own CFO and 160 samples of slack, so the duty cycle is
frame / (frame + 160) and is stated in the record.  Two blocks, N = 64 (29 data symbols: 3120-sample frames, about 600 of them) and
N = 1024 (4 data symbols: 17 920-sample frames, about 110).

Per block, every comparison alternated in this one process, `--reps` passes each after one warm-up, wall clock (the calls are synchronous),
median and spread (max - min):

  find     the loop  d_k = sc_correlate_long(lag_lo = d_{k-1} + frame - W - L)  until nothing is found, against ONE
           sc_scan_long(holdoff = frame - W).  Asserted in the same run: the same d_hat list, f_delta within 1e-9, metric within 1e-6.
  decode   the loop of tests/test_gpu_host_path.py, decode_long(lag_lo = end of the last packet), against the scan followed by
           decode_long(lag_lo = where the search for packet k started) per detection (api.decode_all's way).  Asserted: bytes, length,
           status and offset of every packet equal, f_delta within 1e-9 and metric within 1e-6 (recorded: whether bit for bit).  Both
           decode one packet per call: the scan removes the dependence of one call on the one before, not the calls.
  mark     k_sc_mark alone over every lag (laboratory key scan_mark_only; the context's event timer) in lags per second and in bytes of
           capture per second, against ofdm_hbm_read_probe (unit-stride 16-byte loads) over the same bytes.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, link, median, open_record  # noqa: E402


def stat(ms):
    return {"ms_all": [round(v, 4) for v in ms], "ms_median": round(median(ms), 4), "ms_spread": round(max(ms) - min(ms), 4)}


def wall_alternated(runs, reps):
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def block(n_fft, data_symbols, samples, reps, seed):
    probe = api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True)
    payload = data_symbols * probe.bytes_per_symbol - 16
    frame = probe.frame_samples(payload)
    rows = samples // (frame + 160) + 1
    c, pay, rx, D = link(api.ECC_NONE, n_fft, api.QAM64, rows, payload, 30.0, seed)
    assert D == data_symbols and rx.shape[1] == frame + 160
    x = rx.reshape(-1)[:samples].contiguous()
    L, W = c.S, c.params.sync_window_reps * c.S
    holdoff = frame - W
    out = {}

    def find_loop():
        got, lo = [], 0
        while True:
            d, fd, m = c.sc_correlate_long(x, lag_lo=lo)
            if d < 0:
                break
            got.append((d, fd, m))
            lo = d + frame - W - L
        out["find_loop"] = got

    def find_scan():
        out["find_scan"] = c.sc_scan_long(x, holdoff, 1 << 16)

    def decode_loop():
        got, lo = [], 0
        while True:
            r = c.decode_long(x, D, lag_lo=lo)
            if r["status"] == api.FRAME_NOSYNC:
                break
            got.append(r)
            lo = max(lo + 1, r["offset"] + frame)
        out["decode_loop"] = got

    def decode_scan():
        det = c.sc_scan_long(x, holdoff, 1 << 16)
        out["decode_scan"] = [c.decode_long(x, D, lag_lo=int(lo)) for lo in det["lag_lo"]]

    ms = wall_alternated({"find_loop": find_loop, "find_scan": find_scan}, reps)
    scan_dispatch = c.last_dispatch()
    loop, scan = out["find_loop"], out["find_scan"]
    same_find = [d for d, _, _ in loop] == scan["d_hat"].tolist() and not scan["more"] and \
        all(abs(fd - a) <= 1e-9 and abs(m - float(b)) <= 1e-6 for (_, fd, m), a, b in zip(loop, scan["f_delta"], scan["metric"]))
    assert same_find, "the scan and the loop of sc_correlate_long found different packets"
    rec = {"n_fft": n_fft, "samples": samples, "frame_samples": frame, "data_symbols": data_symbols, "payload_bytes": payload,
           "duty_cycle": round(frame / (frame + 160), 4), "packets_found": len(loop), "holdoff": holdoff, "scan_dispatch": scan_dispatch,
           "find": {"loop_of_sc_correlate_long": stat(ms["find_loop"]), "sc_scan_long": stat(ms["find_scan"]), "outputs_equal": bool(same_find)}}
    rec["find"]["ratio_loop_over_scan"] = round(rec["find"]["loop_of_sc_correlate_long"]["ms_median"] / rec["find"]["sc_scan_long"]["ms_median"], 2)

    ms = wall_alternated({"decode_loop": decode_loop, "decode_scan": decode_scan}, reps)
    a, b = out["decode_loop"], out["decode_scan"]
    same = len(a) == len(b) and all(p[k] == q[k] for p, q in zip(a, b) for k in ("len", "status", "offset")) and \
        all(abs(p["f_delta"] - q["f_delta"]) <= 1e-9 and abs(p["metric"] - q["metric"]) <= 1e-6 for p, q in zip(a, b)) and \
        all(torch.equal(p["bytes"][: p["len"]], q["bytes"][: q["len"]]) for p, q in zip(a, b))
    bit_same = all(p[k] == q[k] for p, q in zip(a, b) for k in ("f_delta", "metric"))
    assert same, "the scan-led decode and the loop of decode_long delivered different packets"
    sent = sum(int(r["status"] == 0 and r["len"] == payload and torch.equal(r["bytes"][:payload], pay[k])) for k, r in enumerate(b))
    rec["decode"] = {"loop_of_decode_long": stat(ms["decode_loop"]), "scan_then_decode_long": stat(ms["decode_scan"]), "outputs_equal": bool(same),
                     "f_delta_and_metric_bit_identical": bool(bit_same), "packets": len(b), "payloads_delivered_exactly": sent,
                     "note": "payloads_delivered_exactly counts what the uncoded 64-QAM link delivered whole (the last frame is cut by the "
                             "capture's end; at N = 1024 the data symbols see about 12 dB less than the channel's 30 dB), not what was found"}
    rec["decode"]["ratio_loop_over_scan"] = round(rec["decode"]["loop_of_decode_long"]["ms_median"] / rec["decode"]["scan_then_decode_long"]["ms_median"], 2)

    lags = samples - W - L + 1
    c.set_tuning("scan_mark_only", 1)
    mark = alternated_ms({"k_sc_mark": (c, lambda: c.sc_scan_long(x, holdoff, 1)),
                          "hbm_read_probe": (c, lambda: c.hbm_read_probe(x[: (samples // 80) * 80], 2))}, reps)
    c.set_tuning("scan_mark_only", 0)
    km, pm = stat(mark["k_sc_mark"]), stat(mark["hbm_read_probe"])
    rec["mark"] = {"lags": lags, "k_sc_mark": {**km, "glags_per_s": round(lags / km["ms_median"] / 1e6, 3),
                                               "capture_gbytes_per_s": round(8 * samples / km["ms_median"] / 1e6, 2)},
                   "hbm_read_probe": {**pm, "capture_gbytes_per_s": round(8 * samples / pm["ms_median"] / 1e6, 2)},
                   "ratio_mark_over_probe": round(km["ms_median"] / pm["ms_median"], 1)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="n64,n1024")
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_scan.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process; per comparison one warm-up of every variant, then alternated passes; wall clock (k_sc_mark and the read "
                     "probe: the context's event timer); median and spread (max - min)"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    for name, n_fft, syms, seed in (("n64", 64, 29, 1201), ("n1024", 1024, 4, 1202)):
        if name in a.blocks.split(","):
            rec[name] = block(n_fft, syms, a.samples, a.reps, seed)
            save()
            torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
