"""The RS-outer frame modes (OFDM_ECC_RS255 = 20 + inner) against their inner modes: frames delivered, air time and speed.  Prints one
JSON record and writes it to profiles/rs_ber_and_speed.json (--out).

  delivery  the seeded link of tools/link.py: N = 64, payload 560, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay
            1..32, CFO), the same payloads, delays, CFO and channel seed for every mode, every mode encoded by its own context.  Per
            point and mode: frames delivered right (status 0, the true length -- for an RS mode the payload zero-padded to whole
            blocks, trailing zero block included -- and every byte), frames delivered WRONG with status 0, frames reported
            (OFDM_FRAME_HEADER / OFDM_FRAME_UNCORRECTABLE), other statuses, and the frame's samples.
  speed     262 144 N = 64 frames (payload 560) and config 4 (N = 1024, payload 1304, 65 536 frames).  An RS mode's frame IS its inner
            mode's frame of the RS-coded bytes, so each pair decodes the SAME capture: the inner context sees a payload of
            255 (p / 223 + 1) bytes, the RS context the p bytes inside.  The eight passes are alternated in one process after a
            warm-up of all; device-event ms per pass, median of --reps, with the spread of the inner passes.
  kernel    k_rs255_decode alone (ofdm_rs255_decode_batch) over the same number of rows of the same length, clean and with 8 byte
            errors in every block, and the host ofdm_rs255_decode over the same bytes on --host-threads CPU threads.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, capture, delivered, link, link_on, median, open_record  # noqa: E402

INNER = (("none", api.ECC_NONE), ("k7f_r12", api.ECC_CONV_K7F_R12), ("k7f_r23", api.ECC_CONV_K7F_R23), ("k7f_r34", api.ECC_CONV_K7F_R34))


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


def delivery(n, payload, snrs, n_frames, seed):
    modes = [(name, ecc) for name, ecc in INNER] + [("rs_" + name, 20 + ecc) for name, ecc in INNER]
    ctxs = {name: _ctx(n, ecc) for name, ecc in modes}
    padded = 223 * (255 * (payload // 223 + 1) // 255 + 1)
    rows = []
    for snr in snrs:
        row = {"snr_db": snr}
        for name, c in ctxs.items():
            pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            r = c.decode_batch(rx, max_symbols=c.data_symbols(payload))
            torch.cuda.synchronize()
            del rx
            rs = name.startswith("rs_")
            right, ok = delivered(r, pay, padded if rs else payload)
            if rs:
                right &= ~(r["bytes"][:, payload:padded] != 0).any(dim=1)
            reported = (r["status"] == api.FRAME_HEADER) | (r["status"] == api.FRAME_UNCORRECTABLE)
            row[name] = {"delivered_right": int(right.sum()), "delivered_wrong_status_0": int((ok & ~right).sum()),
                         "reported": int(reported.sum()), "uncorrectable": int((r["status"] == api.FRAME_UNCORRECTABLE).sum()),
                         "other_status": int(((r["status"] != 0) & ~reported).sum()), "frame_samples": c.frame_samples(payload)}
        rows.append(row)
        torch.cuda.empty_cache()
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample",
            "caveat": "frames of different length see slightly different noise at equal snr_db (the noise is scaled by the whole frame's "
                      "pseudo-variance)", "points": rows}


def test_point(snrs, n_frames=256, payload=560, seed=9012):
    """the counts of tests/test_gpu_rs.py::test_rs_outer_code_earns_its_keep over the link that test runs (tools/link.py: N = 64,
    64-QAM, guard bands): frames not delivered right by rate 3/4 alone and with RS around it, and RS-mode frames delivered wrong
    with status 0"""
    rows = []
    for snr in snrs:
        row = {"snr_db": snr, "frames": n_frames, "payload": payload, "seed": seed}
        for name, ecc in (("k7f_r34", api.ECC_CONV_K7F_R34), ("rs_k7f_r34", api.ECC_RS255_K7F_R34)):
            c, pay, rx, D = link(ecc, 64, api.QAM64, n_frames, payload, snr, seed)
            r = c.decode_batch(rx, max_symbols=D)
            torch.cuda.synchronize()
            right, ok = delivered(r, pay, payload if ecc < 20 else 223 * (255 * (payload // 223 + 1) // 255 + 1))
            row[name] = {"not_delivered_right": int((~right).sum()), "wrong_with_status_0": int((ok & ~right).sum())}
        rows.append(row)
    return rows


def _host_decode(lib, rows, threads):
    """wall-clock seconds of ofdm_rs255_decode over every row, the rows shared out over `threads` threads; (seconds, rows it failed)"""
    n, width = rows.shape
    out_w = 223 * (width // 255 + 1)

    def work(lo, hi):
        out = np.zeros(out_w, np.uint8)
        bad = 0
        for f in range(lo, hi):
            bad += lib.ofdm_rs255_decode(C.c_void_p(rows[f].ctypes.data), width, C.c_void_p(out.ctypes.data), None) != 0
        return bad

    step = (n + threads - 1) // threads
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        bad = sum(ex.map(lambda lo: work(lo, min(lo + step, n)), range(0, n, step)))
    return time.perf_counter() - t0, int(bad)


def kernel_alone(c, n_rows, payload, reps, threads):
    g = torch.Generator(device=c.device); g.manual_seed(8)
    pay = torch.randint(0, 256, (n_rows, payload), dtype=torch.uint8, device=c.device, generator=g)
    clean = c.rs255_encode(pay)
    width, blocks = clean.shape[1], clean.shape[1] // 255
    # 8 errors a block: positions base + 31 j (mod 255, distinct), a non-zero value each
    base = torch.randint(0, 255, (n_rows, blocks, 1), device=c.device, generator=g)
    pos = (base + 31 * torch.arange(8, device=c.device).view(1, 1, 8)) % 255 + 255 * torch.arange(blocks, device=c.device).view(1, blocks, 1)
    val = torch.randint(1, 256, (n_rows, blocks * 8), dtype=torch.uint8, device=c.device, generator=g)
    dirty = clean.clone()
    idx = pos.reshape(n_rows, blocks * 8)
    dirty.scatter_(1, idx, torch.bitwise_xor(torch.gather(dirty, 1, idx), val))
    res = {"rows": n_rows, "row_bytes": width, "blocks_per_row": blocks + 1, "host_threads": threads}
    for name, code in (("clean", clean), ("errors_8_per_block", dirty)):
        ms = alternated_ms({"decode": (c, lambda: c.rs255_decode(code))}, reps)["decode"]
        out, out_len, fixed = c.rs255_decode(code)
        ok = bool((out[:, :payload] == pay).all()) and bool((fixed == (0 if name == "clean" else 8 * blocks)).all())
        host_s, host_bad = _host_decode(c.lib, code.cpu().numpy(), threads)
        res[name] = {"k_rs255_decode_ms": median(ms), "ms_all": ms, "device_output_right": ok, "host_ms": 1e3 * host_s,
                     "host_rows_failed": host_bad, "host_over_device": 1e3 * host_s / median(ms)}
    res["k_rs255_encode_ms"] = median(alternated_ms({"encode": (c, lambda: c.rs255_encode(pay))}, reps)["encode"])
    return res


def speed(n, n_frames, payload, reps, threads):
    res = {"n_fft": n, "frames": n_frames, "payload": payload, "inner_bytes": 255 * (payload // 223 + 1)}
    runs = {}
    for name, ecc in INNER:
        c, ci = _ctx(n, 20 + ecc), _ctx(n, ecc)
        g = torch.Generator(device=c.device); g.manual_seed(4)
        pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=c.device, generator=g)
        D = c.data_symbols(payload)
        assert D == ci.data_symbols(res["inner_bytes"])
        x = capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003)
        runs["rs_" + name], runs[name] = (c, x, D, pay), (ci, x, D, None)
    # warm-up of all, then alternated: rs_none, none, rs_k7f_r12, k7f_r12, ...
    times = alternated_ms({name: (c, lambda c=c, x=x, D=D: c.decode_batch(x, max_symbols=D)) for name, (c, x, D, _) in runs.items()}, reps)
    padded = 223 * (res["inner_bytes"] // 255 + 1)
    for name, (c, x, D, pay) in runs.items():
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        res[name] = {"ms_per_pass": median(times[name]), "ms_all": times[name], "spread_ms": max(times[name]) - min(times[name]),
                     "data_symbols": D, "frame_samples": c.frame_samples(payload if pay is not None else res["inner_bytes"]),
                     "dispatch": c.last_dispatch()}
        if pay is not None:
            ok = (r["status"] == 0) & (r["len"] == padded)
            res[name]["frames_exact"] = int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())
        else:
            res[name]["frames_status_0"] = int(((r["status"] == 0) & (r["len"] == res["inner_bytes"])).sum())
    for name, _ in INNER:
        res["rs_" + name]["minus_inner_ms"] = res["rs_" + name]["ms_per_pass"] - res[name]["ms_per_pass"]
        res["rs_" + name]["over_inner"] = res["rs_" + name]["ms_per_pass"] / res[name]["ms_per_pass"]
    c0 = runs["rs_none"][0]
    del runs
    torch.cuda.empty_cache()
    res["kernel_alone"] = kernel_alone(c0, n_frames, payload, reps, threads)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--delivery-only", action="store_true")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096, help="frames per point of the delivery table")
    ap.add_argument("--snrs", default="8,9,10,11,12,13,14,15,16", help="dB, channel.rs definition")
    ap.add_argument("--shapes", default="n64,cfg4", help="speed blocks to run")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_rs.py", "llr_scale": api.SOFT_LLR_SCALE, "device": torch.cuda.get_device_name(0),
           "definition": "ofdm_rs255_decode (ofdm_amd/csrc/outer_code.hip), pinned to the oracle's decipher_transmission_bytes"}
    rec, save = open_record(rec, a.out)   # saved after every block: a long run that is cut short keeps what it has
    if not a.speed_only:
        rec["test_rs_outer_code_earns_its_keep"] = test_point([12.0, 11.0, 13.0])
        rec["delivery"] = delivery(64, 560, [float(v) for v in a.snrs.split(",")], a.frames, 11)
        save()
    if not a.delivery_only:
        shapes = {"cfg4": lambda: speed(1024, a.cfg4_frames, 1304, a.reps, a.host_threads),
                  "n64": lambda: speed(64, a.n64_frames, 560, a.reps, a.host_threads)}
        rec["speed"] = {}
        for k in a.shapes.split(","):
            rec["speed"][k] = shapes[k]()
            save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
