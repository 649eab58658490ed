"""The framed convolutional modes (OFDM_ECC_CONV_K7F_R12 / _R23 / _R34) against OFDM_ECC_CONV_K7: frames delivered, BER, air time and
speed.  Prints one JSON record and writes it to profiles/framed_ber_and_speed.json (--out).  These modes are parity unpinned by the
reference: tests/framed_ref.py is the definition.

  ber    N = 64 and N = 1024, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32, CFO), the SNR grids of
         tools/bench_conv.py: the same payloads, delays, CFO and channel seed for the four decoders, every mode encoded by its own
         context.  Per point and mode: frames_ok (status 0 and the true length), invalid length blocks (status OFDM_FRAME_HEADER;
         CONV_K7 has no such report: a garbled header gives a wrong length or a cut frame there), status 0 with a wrong length, and
         payload bit errors over the frames that ALL FOUR decode (frames_compared).  Frames of different length see slightly
         different noise at equal snr_db: ofdm_channel_batch scales its noise by the whole frame's pseudo-variance, and the pilot-only
         header symbols weigh differently in a shorter frame (README, "soft decisions").
  speed  config 4 (N = 1024, payload 1304, 65 536 frames) and N = 64 (payload 560): the decode pass of the four modes, each on its
         own capture of the same payloads, alternated in one process after a warm-up of all; device-event ms per pass.  The framed
         rate-1/2 pass does the body work of CONV_K7 plus 72 steps per frame: compare it with the CONV_K7 pass OF THE SAME RUN and
         with the spread of that run's CONV_K7 passes (conv_k7_spread_ms).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, bit_errors, capture, link_on, median, save_record  # noqa: E402

MODES = (("conv_k7", api.ECC_CONV_K7), ("k7f_r12", api.ECC_CONV_K7F_R12), ("k7f_r23", api.ECC_CONV_K7F_R23),
         ("k7f_r34", api.ECC_CONV_K7F_R34))


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


def air_time(n, payload):
    out = {}
    for name, ecc in MODES:
        c = _ctx(n, ecc)
        out[name] = {"coded_len": c.coded_len(payload), "data_symbols": c.data_symbols(payload), "frame_samples": c.frame_samples(payload)}
    return out


def ber(n, payload, snrs, n_frames, seed):
    ctxs = {name: _ctx(n, ecc) for name, ecc in MODES}
    rows = []
    for snr in snrs:
        row, res, oks = {"snr_db": snr}, {}, {}
        for name, c in ctxs.items():
            pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            r = c.decode_batch(rx, max_symbols=c.data_symbols(payload))
            torch.cuda.synchronize()
            del rx
            oks[name] = (r["status"] == 0) & (r["len"] == payload)
            res[name] = (r, pay)
        every = oks["conv_k7"] & oks["k7f_r12"] & oks["k7f_r23"] & oks["k7f_r34"]
        row["frames_compared"] = int(every.sum())
        for name in ctxs:
            r, pay = res[name]
            diff = torch.bitwise_xor(r["bytes"][:, :payload], pay)
            bits = bit_errors(diff[every])
            whole = oks[name] & (diff == 0).all(dim=1)
            row[name] = {"frames_ok": int(oks[name].sum()), "frames_delivered_whole": int(whole.sum()),
                         "invalid_length_blocks": int((r["status"] == api.FRAME_HEADER).sum()),
                         "status_ok_wrong_length": int(((r["status"] == 0) & (r["len"] != payload)).sum()),
                         "payload_bit_errors": bits, "ber": bits / max(1, row["frames_compared"] * payload * 8),
                         "frames_with_errors": int((diff[every] != 0).any(dim=1).sum())}
        rows.append(row)
        del res
        torch.cuda.empty_cache()
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample",
            "caveat": "frames of different length see slightly different noise at equal snr_db (the noise is scaled by the whole frame's "
                      "pseudo-variance)", "air_time": air_time(n, payload), "points": rows}


def speed(n, n_frames, payload, reps):
    res = {"n_fft": n, "frames": n_frames, "payload": payload}
    caps = {}
    for name, ecc in MODES:
        c = _ctx(n, ecc)
        g = torch.Generator(device=c.device); g.manual_seed(4)
        pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=c.device, generator=g)
        D = c.data_symbols(payload)
        caps[name] = (c, capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003), D, pay)
    # warm-up of all, then alternated: conv_k7, k7f_r12, k7f_r23, k7f_r34, conv_k7 ...
    times = alternated_ms({name: (c, lambda c=c, x=x, D=D: c.decode_batch(x, max_symbols=D)) for name, (c, x, D, _) in caps.items()}, reps)
    for name, (c, x, D, pay) in caps.items():
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        m = median(times[name])
        ok = (r["status"] == 0) & (r["len"] == payload)
        res[name] = {"ms_per_pass": m, "ms_all": times[name], "data_symbols": D, "coded_len": c.coded_len(payload),
                     "frame_samples": c.frame_samples(payload), "dispatch": c.last_dispatch(),
                     "frames_exact": int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())}
    base = res["conv_k7"]
    res["conv_k7_spread_ms"] = max(base["ms_all"]) - min(base["ms_all"])
    res["k7f_r12_minus_conv_k7_ms"] = res["k7f_r12"]["ms_per_pass"] - base["ms_per_pass"]
    for name in ("k7f_r12", "k7f_r23", "k7f_r34"):
        res[name]["over_conv_k7"] = res[name]["ms_per_pass"] / base["ms_per_pass"]
    del caps
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed-only", action="store_true")
    ap.add_argument("--ber-only", action="store_true")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ber-frames", type=int, default=4096)
    ap.add_argument("--snrs", default="8,10,12,14,16,18,20,22", help="N = 64 grid (dB, channel.rs definition)")
    ap.add_argument("--snrs-1024", default="22,24,26,28,30,32,34,36,38,40", help="N = 1024 grid (see tools/bench_soft.py)")
    ap.add_argument("--shapes", default="cfg4,n64", help="speed blocks to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framed_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_framed.py", "llr_scale": api.SOFT_LLR_SCALE, "device": torch.cuda.get_device_name(0),
           "definition": "parity unpinned by the reference: tests/framed_ref.py is the definition"}
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
