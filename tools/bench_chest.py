"""EXT-5 channel-estimate denoising (chest_mode = OFDM_CHEST_WLS) against the reference's estimate (OFDM_CHEST_LS): what it delivers and
what it costs.  Prints one JSON record and writes it to profiles/chest_ber_and_speed.json (--out).  The stage is parity unpinned by the
reference: tests/chest_ref.py is the definition.

  ber    N = 64 (8 .. 16 dB) and N = 1024 (26 .. 38 dB), 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32,
         CFO): per point and ecc ONE capture -- the same payloads, delays, CFO, snr_db and channel seed -- decoded by a context with the
         mode off and one with it on.  Per point, ecc and mode: frames right (status 0, the true length, every byte), wrong (status 0
         otherwise), reported (status != 0), and payload bit errors over the frames that BOTH modes deliver with the true length
         (frames_compared).  RS modes deliver whole 223-byte blocks: the true length is 223 (p / 223 + 1), the payload its head.
  speed  config 4 (N = 1024, payload 1304, 65 536 frames) and N = 64 (payload 560, 262 144 frames), ecc NONE and HAMMING74 (the two
         whose default chain is a fused frame kernel, which the mode cannot use) and HAMMING74_SOFT (generic chain either way): the
         decode pass with the mode off against on, alternated in one process after a warm-up of both, device-event ms per pass.
         Then the stage alone (ofdm_chest_smooth_batch) and k_chest_solve alone (laboratory key chest_solve_only) on that many rows,
         with the kernel's rate: 8 n_frames L_h^2 flop.
  host   ofdm_chest_matrix per N (the f64 Toeplitz solve ofdm_create runs when the mode is on): best of three, ms.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, bit_errors, capture, link_on, median, save_record  # noqa: E402

BER_MODES = (("none", api.ECC_NONE), ("hamming74_soft", api.ECC_HAMMING74_SOFT), ("k7f_r12", api.ECC_CONV_K7F_R12),
             ("k7f_r23", api.ECC_CONV_K7F_R23), ("k7f_r34", api.ECC_CONV_K7F_R34), ("rs255_k7f_r34", api.ECC_RS255_K7F_R34))
SPEED_MODES = (("none", api.ECC_NONE), ("hamming74", api.ECC_HAMMING74), ("hamming74_soft", api.ECC_HAMMING74_SOFT))
CHEST = (("ls", api.CHEST_LS), ("wls", api.CHEST_WLS))
PEAK_F32_TFLOPS = 157.3


def _ctx(n, ecc, chest):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc, chest_mode=chest)


def ber(n, payload, snrs, n_frames, seed):
    rows = []
    for snr in snrs:
        row = {"snr_db": snr}
        for name, ecc in BER_MODES:
            ctxs = {k: _ctx(n, ecc, v) for k, v in CHEST}
            c = ctxs["ls"]
            pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            true_len = 223 * (payload // 223 + 1) if ecc == api.ECC_RS255_K7F_R34 else payload
            res = {k: cx.decode_batch(rx, max_symbols=c.data_symbols(payload)) for k, cx in ctxs.items()}
            torch.cuda.synchronize()
            del rx
            oks = {k: (r["status"] == 0) & (r["len"] == true_len) for k, r in res.items()}
            both = oks["ls"] & oks["wls"]
            row[name] = {"frames_compared": int(both.sum())}
            for k, r in res.items():
                diff = torch.bitwise_xor(r["bytes"][:, :payload], pay)
                right = oks[k] & (diff == 0).all(dim=1)
                bits = bit_errors(diff[both])
                row[name][k] = {"frames_right": int(right.sum()), "frames_wrong": int(((r["status"] == 0) & ~right).sum()),
                                "frames_reported": int((r["status"] != 0).sum()), "payload_bit_errors": bits,
                                "ber": bits / max(1, int(both.sum()) * payload * 8)}
            del res
            torch.cuda.empty_cache()
        print(f"ber n_fft {n} snr {snr}: done", file=sys.stderr, flush=True)
        rows.append(row)
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample", "points": rows}


def speed(n, n_frames, payload, reps):
    res = {"n_fft": n, "frames": n_frames, "payload": payload}
    for name, ecc in SPEED_MODES:
        ctxs = {k: _ctx(n, ecc, v) for k, v in CHEST}
        c = ctxs["ls"]
        g = torch.Generator(device=c.device); g.manual_seed(4)
        pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=c.device, generator=g)
        D = c.data_symbols(payload)
        x = capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003)
        # warm-up of both (tables, workspaces, code objects), then alternated: ls, wls, ls, ...
        times = alternated_ms({k: (cx, lambda cx=cx, x=x: cx.decode_batch(x, max_symbols=D)) for k, cx in ctxs.items()}, reps)
        out = {}
        for k, cx in ctxs.items():
            r = cx.decode_batch(x, max_symbols=D)
            torch.cuda.synchronize()
            ok = (r["status"] == 0) & (r["len"] == payload)
            out[k] = {"ms_per_pass": median(times[k]), "ms_all": times[k], "dispatch": cx.last_dispatch(),
                      "frames_exact": int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())}
            del r
        out["wls_minus_ls_ms"] = out["wls"]["ms_per_pass"] - out["ls"]["ms_per_pass"]
        out["wls_over_ls"] = out["wls"]["ms_per_pass"] / out["ls"]["ms_per_pass"]
        res[name] = out
        del x, ctxs
        torch.cuda.empty_cache()
        print(f"speed n_fft {n} {name}: done", file=sys.stderr, flush=True)
    # the stage and its contraction alone, on that many rows of a plausible estimate
    c = _ctx(n, api.ECC_NONE, api.CHEST_LS)
    hk = torch.randn((n_frames, n), dtype=torch.complex64, device=c.device)
    out = torch.empty_like(hk)
    stage = {}
    for key, solve_only in (("stage_ms", 0), ("k_chest_solve_ms", 1)):
        c.set_tuning("chest_solve_only", solve_only)
        t = alternated_ms({key: (c, lambda: c.chest_smooth(hk, out=out))}, reps)[key]
        stage[key] = median(t)
        stage[key + "_all"] = t
        stage[key.replace("_ms", "_dispatch")] = c.last_dispatch()
    c.set_tuning("chest_solve_only", 0)
    flop = 8.0 * n_frames * (n // 4) ** 2
    stage["k_chest_solve_gflop"] = flop / 1e9
    stage["k_chest_solve_tflops"] = flop / (stage["k_chest_solve_ms"] * 1e-3) / 1e12
    stage["k_chest_solve_fraction_of_f32_peak"] = stage["k_chest_solve_tflops"] / PEAK_F32_TFLOPS
    res["stage"] = stage
    del hk, out
    torch.cuda.empty_cache()
    return res


def host_solve():
    lib = api._lib.load()
    rows = []
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        buf = np.zeros((n // 4, n // 4), np.complex128)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            rc = lib.ofdm_chest_matrix(n, n // 4, None, C.c_void_p(buf.ctypes.data))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            best = dt if best is None else min(best, dt)
        rows.append({"n_fft": n, "taps": n // 4, "ofdm_chest_matrix_ms": best})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--ber-only", action="store_true")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ber-frames", type=int, default=4096)
    ap.add_argument("--snrs", default="8,10,12,14,16", help="N = 64 grid (dB, channel.rs definition)")
    ap.add_argument("--snrs-1024", default="26,28,30,32,34,36,38", help="N = 1024 grid")
    ap.add_argument("--shapes", default="cfg4,n64", help="speed blocks to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chest_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_chest.py", "device": torch.cuda.get_device_name(0),
           "definition": "parity unpinned by the reference: tests/chest_ref.py is the definition", "host_solve": host_solve()}
    if not a.ber_only:
        shapes = {"cfg4": lambda: speed(1024, a.cfg4_frames, 1304, a.reps), "n64": lambda: speed(64, a.n64_frames, 560, a.reps)}
        rec["speed"] = {k: shapes[k]() for k in a.shapes.split(",")}
    if not a.speed_only:
        rec["ber"] = [ber(64, 560, [float(v) for v in a.snrs.split(",")], a.ber_frames, 11),
                      ber(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.ber_frames, 12)]
    print(json.dumps(rec))
    save_record(rec, a.out)


if __name__ == "__main__":
    main()
