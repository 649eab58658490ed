"""The frame-check modes (OFDM_ECC_FCS + mode = 64 + mode) against their base modes: frames right / wrong / reported, and speed.  Prints
one JSON record and writes it to profiles/fcs_ber_and_speed.json (--out).

  link      the seeded link of tools/link.py: N = 64, payload 560, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay
            1..32, CFO), the same payloads, delays, CFO and channel seed for every mode, every mode encoded by its own context.  Per
            point and mode: frames right (status 0, the true length and every byte; a base mode that pads -- Hamming -- is right when
            its first 560 bytes are), frames WRONG with status 0, frames reported (any other status; those of the check separately).
            The point of the exercise is the `wrong` column of the FCS modes.
  speed     262 144 N = 64 frames (payload 560) and config 4 (N = 1024, payload 1304, 65 536 frames).  An FCS mode's frame IS its base
            mode's frame of the envelope, so each pair decodes the SAME capture: the base context sees a payload of p + 8 bytes, the
            FCS context the p bytes inside.  One pair at a time: warm-up of both, then the two passes alternated --reps times;
            device-event ms per pass, median, with the spread of the passes.
  kernel    k_fcs_check and k_fcs_wrap alone (ofdm_fcs_check_batch / ofdm_fcs_wrap_batch) over the same number of rows of the same
            length, with the slice-by-4 tables and bit-serial (laboratory key fcs_bitserial), and the host ofdm_crc32 over the same
            bytes on --host-threads CPU threads; the device's check words are compared with the host's in the same run.
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
from tools.link import alternated_ms, capture, delivered, link_on, median, open_record  # noqa: E402

BASE = (("none", api.ECC_NONE), ("hamming74_soft", api.ECC_HAMMING74_SOFT), ("conv_k7", api.ECC_CONV_K7), ("k7f_r12", api.ECC_CONV_K7F_R12),
        ("k7f_r23", api.ECC_CONV_K7F_R23), ("k7f_r34", api.ECC_CONV_K7F_R34))


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


def link(n, payload, snrs, n_frames, seed):
    modes = [(name, ecc) for name, ecc in BASE] + [("fcs_" + name, api.ECC_FCS + ecc) for name, ecc in BASE]
    ctxs = {name: _ctx(n, ecc) for name, ecc in modes}
    rows = []
    for snr in snrs:
        row = {"snr_db": snr}
        for name, c in ctxs.items():
            pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            r = c.decode_batch(rx, max_symbols=c.data_symbols(payload))
            torch.cuda.synchronize()
            del rx
            exact = name.startswith("fcs_") or "hamming" not in name      # Hamming alone delivers floor(coded / 7) * 4 >= payload bytes
            right, ok = delivered(r, pay, payload, exact)
            row[name] = {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum()),
                         "reported_by_the_check": int((r["status"] == api.FRAME_FCS).sum()), "frame_samples": c.frame_samples(payload)}
        rows.append(row)
        torch.cuda.empty_cache()
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample",
            "caveat": "frames of different length see slightly different noise at equal snr_db (the noise is scaled by the whole frame's "
                      "pseudo-variance)",
            "fcs_modes_wrong_total": sum(v["wrong"] for row in rows for k, v in row.items() if k.startswith("fcs_")), "points": rows}


def _host_crc(lib, rows, width, threads):
    """wall-clock seconds of ofdm_crc32 over the first `width` bytes of every row, shared out over `threads` threads; (seconds, crcs)"""
    n = rows.shape[0]
    out = np.zeros(n, np.uint32)

    def work(lo, hi):
        for f in range(lo, hi):
            out[f] = lib.ofdm_crc32(C.c_void_p(rows[f].ctypes.data), width)

    step = (n + threads - 1) // threads
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: work(lo, min(lo + step, n)), range(0, n, step)))
    return time.perf_counter() - t0, out


def kernel_alone(c, n_rows, payload, reps, threads):
    g = torch.Generator(device=c.device); g.manual_seed(8)
    pay = torch.randint(0, 256, (n_rows, payload), dtype=torch.uint8, device=c.device, generator=g)
    res = {"rows": n_rows, "payload": payload, "row_bytes": payload + api.FCS_OVERHEAD, "host_threads": threads}
    env = None
    for variant, key in (("slice_by_4_lds", 0), ("bit_serial", 1)):
        c.set_tuning("fcs_bitserial", key)
        env = c.fcs_wrap(pay)
        out, out_len, ok = c.fcs_check(env)
        torch.cuda.synchronize()
        ms = alternated_ms({"wrap": (c, lambda: c.fcs_wrap(pay)), "check": (c, lambda: c.fcs_check(env))}, reps)
        wrap_ms, check_ms = ms["wrap"], ms["check"]
        dirty = env.clone()
        dirty[::2, 100] ^= 0x40
        _, dlen, dok = c.fcs_check(dirty)
        torch.cuda.synchronize()
        res[variant] = {"k_fcs_wrap_ms": median(wrap_ms), "k_fcs_check_ms": median(check_ms), "wrap_ms_all": wrap_ms, "check_ms_all": check_ms,
                        "every_clean_row_accepted": bool((ok == 1).all()) and bool((out_len == payload).all()) and bool((out == pay).all()),
                        "every_damaged_row_rejected": bool((dok[::2] == 0).all()) and bool((dok[1::2] == 1).all()) and bool((dlen[::2] == 0).all())}
        del dirty
    c.set_tuning("fcs_bitserial", 0)
    host_rows = env.cpu().numpy()
    host_s, crcs = _host_crc(c.lib, host_rows, payload + 4, threads)
    dev = host_rows[:, payload + 4:].copy().view("<u4").reshape(-1)
    res["host_crc32_ms"] = 1e3 * host_s
    res["device_check_words_equal_host"] = bool(np.array_equal(dev, crcs))
    res["host_over_k_fcs_check"] = 1e3 * host_s / res["slice_by_4_lds"]["k_fcs_check_ms"]
    return res


def speed(n, n_frames, payload, reps, threads, names):
    res = {"n_fft": n, "frames": n_frames, "payload": payload, "base_bytes": payload + api.FCS_OVERHEAD, "reps": reps}
    c0 = None
    for name, ecc in BASE:
        if name not in names:
            continue
        c, cb = _ctx(n, api.ECC_FCS + ecc), _ctx(n, ecc)
        g = torch.Generator(device=c.device); g.manual_seed(4)
        pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=c.device, generator=g)
        D = c.data_symbols(payload)
        assert D == cb.data_symbols(payload + api.FCS_OVERHEAD)
        x = capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003)
        # warm-up of both, then alternated: fcs, base, fcs, base, ...
        ms = alternated_ms({"fcs": (c, lambda: c.decode_batch(x, max_symbols=D)), "base": (cb, lambda: cb.decode_batch(x, max_symbols=D))}, reps)
        t_fcs, t_base = ms["fcs"], ms["base"]
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        right, ok = delivered(r, pay, payload)
        exact, wrong = int(right.sum()), int((ok & ~right).sum())
        res["fcs_" + name] = {"ms_per_pass": median(t_fcs), "ms_all": t_fcs, "spread_ms": max(t_fcs) - min(t_fcs), "data_symbols": D,
                              "frames_exact": exact, "frames_wrong_status_0": wrong, "dispatch": c.last_dispatch(),
                              "minus_base_ms": median(t_fcs) - median(t_base), "over_base": median(t_fcs) / median(t_base)}
        rb = cb.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        res[name] = {"ms_per_pass": median(t_base), "ms_all": t_base, "spread_ms": max(t_base) - min(t_base),
                     "frames_status_0": int((rb["status"] == 0).sum()), "dispatch": cb.last_dispatch()}
        c0 = c0 or c
        del x, r, rb, pay
        torch.cuda.empty_cache()
    if c0 is not None:
        res["kernel_alone"] = kernel_alone(c0, n_frames, payload, reps, threads)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--link-only", action="store_true")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096, help="frames per point of the link table")
    ap.add_argument("--snrs", default="8,9,10,11,12,13,14,15,16", help="dB, channel.rs definition")
    ap.add_argument("--shapes", default="n64,cfg4", help="speed blocks to run")
    ap.add_argument("--modes", default=",".join(name for name, _ in BASE), help="base modes of the speed blocks")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcs_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_fcs.py", "llr_scale": api.SOFT_LLR_SCALE, "device": torch.cuda.get_device_name(0),
           "definition": "tests/fcs_ref.py over zlib.crc32: E(payload) = [u32 LE p] ++ payload ++ [u32 LE crc32 of both]"}
    rec, save = open_record(rec, a.out)   # saved after every block: a long run that is cut short keeps what it has
    if not a.speed_only:
        rec["link"] = link(64, 560, [float(v) for v in a.snrs.split(",")], a.frames, 11)
        save()
    if not a.link_only:
        shapes = {"cfg4": lambda: speed(1024, a.cfg4_frames, 1304, a.reps, a.host_threads, a.modes.split(",")),
                  "n64": lambda: speed(64, a.n64_frames, 560, a.reps, a.host_threads, a.modes.split(","))}
        rec["speed"] = {}
        for k in a.shapes.split(","):
            rec["speed"][k] = shapes[k]()
            save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
