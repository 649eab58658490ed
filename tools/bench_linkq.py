"""EXT-6 link quality (ofdm_rx_quality_batch, Context.link_quality): what it measures on the seeded link and what it costs.  Prints one
JSON record and writes it to profiles/linkq_accuracy_and_speed.json (--out).  The stage is parity unpinned by the reference:
tests/quality_ref.py is the definition.

  accuracy  N = 64 (4 .. 20 dB) and N = 1024 (26 .. 38 dB), 64-QAM, guard bands, ecc NONE, through ofdm_channel_batch (FIR CHANNEL,
            delay 1..32, CFO), 4 096 frames a point: the frames are decoded and measured with the decode's own timing and estimate.
            Per point: the channel's snr_db (the axis of the BER tables), tools/link.py's data_snr of it, and over the frames the
            decode accepted the mean, the standard deviation and the 5 / 95 % points of the measured snr_db, the mean evm_db next to
            minus the mean snr_db, and the mean noise variance and gain.
  speed     config 4 (N = 1024, payload 1304, 65 536 frames) and N = 64 (payload 560, 262 144 frames), ecc NONE: the quality pass
            (estimate_channel + rx_quality on the result of a decode, as link_quality runs them; rx_quality alone as well) next to the
            decode pass on the same capture, alternated in one process after a warm-up of all, device-event ms per pass.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, capture, data_snr, link_on, median, open_record  # noqa: E402


def _ctx(n):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_NONE)


def _stats(v):
    v = v.double()
    q = torch.quantile(v, torch.tensor([0.05, 0.95], dtype=torch.float64, device=v.device))
    return {"mean": float(v.mean()), "std": float(v.std()), "p05": float(q[0]), "p95": float(q[1])}


def accuracy(n, payload, snrs, n_frames, seed):
    rows = []
    c = _ctx(n)
    D = c.data_symbols(payload)
    for snr in snrs:
        pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
        r = c.decode_batch(rx, max_symbols=D)
        q = c.link_quality(rx, r, payload_bytes=payload)
        torch.cuda.synchronize()
        ok = q["valid"] & (r["status"] == 0)
        lin = 10.0 ** (q["snr_db"][ok].double() / 10.0)
        row = {"snr_db": snr, "data_snr": float(data_snr(n, snr)), "frames_measured": int(ok.sum()),
               "frames_exact": int(((r["len"] == payload) & (r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum()),
               "measured_snr_db": _stats(q["snr_db"][ok]), "snr_db_of_mean_linear": float(10.0 * torch.log10(lin.mean())),
               "evm_db": _stats(q["evm_db"][ok]), "minus_mean_snr_db": -float(q["snr_db"][ok].double().mean()),
               "noise_var_mean": float(q["noise_var"][ok].double().mean()), "gain_mean": float(q["gain"][ok].double().mean()),
               "points_per_frame": float(q["points"][ok].double().mean())}
        rows.append(row)
        del rx, r, q
        torch.cuda.empty_cache()
        print(f"accuracy n_fft {n} snr {snr}: measured {row['measured_snr_db']['mean']:.2f} dB, evm {row['evm_db']['mean']:.2f} dB", file=sys.stderr, flush=True)
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "ecc": "none", "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample", "points": rows}


def speed(n, n_frames, payload, reps):
    c = _ctx(n)
    g = torch.Generator(device=c.device); g.manual_seed(4)
    pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=c.device, generator=g)
    D = c.data_symbols(payload)
    x = capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003)
    r = c.decode_batch(x, max_symbols=D)
    torch.cuda.synchronize()
    n_points = torch.full((n_frames,), c.frame_points(payload), dtype=torch.int32, device=c.device)
    hk = c.estimate_channel(x, r["offset"], r["f_delta"])
    out = c.empty((n_frames, api.QUALITY_FIELDS), torch.float32)
    runs = {
        "decode": (c, lambda: c.decode_batch(x, max_symbols=D)),
        "link_quality": (c, lambda: c.link_quality(x, r, n_points=n_points)),
        "rx_quality": (c, lambda: c.rx_quality(x, D, 10, n_points, r["offset"], r["f_delta"], hk, r["status"], out=out)),
        "rx_quality_training_only": (c, lambda: c.rx_quality(x, 0, 10, None, r["offset"], r["f_delta"], hk, r["status"], out=out)),
    }
    times = alternated_ms(runs, reps)
    res = {"n_fft": n, "frames": n_frames, "payload": payload, "data_symbols": D, "capture_mb": x.numel() * 8 / 1e6}
    for k, (cx, f) in runs.items():
        f()
        res[k] = {"ms_per_pass": median(times[k]), "ms_all": times[k], "dispatch": cx.last_dispatch()}
    q = c.link_quality(x, r, n_points=n_points)
    torch.cuda.synchronize()
    ok = q["valid"]
    res["frames_measured"] = int(ok.sum())
    res["measured_snr_db_mean"] = float(q["snr_db"][ok].double().mean())
    res["rx_quality_over_decode"] = res["rx_quality"]["ms_per_pass"] / res["decode"]["ms_per_pass"]
    res["link_quality_over_decode"] = res["link_quality"]["ms_per_pass"] / res["decode"]["ms_per_pass"]
    res["rx_quality_gb_per_s_of_frame_samples"] = n_frames * (5 + D) * n * 8 / 1e9 / (res["rx_quality"]["ms_per_pass"] * 1e-3)
    print(f"speed n_fft {n}: decode {res['decode']['ms_per_pass']:.3f} ms, rx_quality {res['rx_quality']['ms_per_pass']:.3f} ms", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--accuracy-only", action="store_true")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096, help="frames per accuracy point")
    ap.add_argument("--snrs", default="4,8,12,16,20", help="N = 64 grid (dB, channel.rs definition)")
    ap.add_argument("--snrs-1024", default="26,28,30,32,34,36,38", help="N = 1024 grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkq_accuracy_and_speed.json"))
    a = ap.parse_args()
    rec, save = open_record({"tool": "tools/bench_linkq.py", "device": torch.cuda.get_device_name(0),
                             "definition": "parity unpinned by the reference: tests/quality_ref.py is the definition"}, a.out, keep_earlier=True)
    if not a.accuracy_only:
        rec["speed"] = {"n64": speed(64, a.n64_frames, 560, a.reps)}
        save()
        rec["speed"]["cfg4"] = speed(1024, a.cfg4_frames, 1304, a.reps)
        save()
    if not a.speed_only:
        rec["accuracy"] = [accuracy(64, 560, [float(v) for v in a.snrs.split(",")], a.frames, 21)]
        save()
        rec["accuracy"].append(accuracy(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.frames, 22))
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
