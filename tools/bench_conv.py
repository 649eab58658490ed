"""The convolutional mode (OFDM_ECC_CONV_K7) against Hamming(7,4), hard and soft: BER and speed.  Prints one JSON record and writes it
to profiles/conv_ber_and_speed.json (--out).

  ber    N = 64 and N = 1024, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32, CFO), the SNR grids of
         tools/bench_soft.py: the same payloads, delays, CFO and channel seed for the three decoders (HAMMING74, HAMMING74_SOFT,
         CONV_K7; the convolutional frames are encoded by their own context -- they are longer).  Payload bit errors over the frames
         that ALL THREE report FRAME_OK with the true length (frames_compared), and header mismatches: frames that some but not
         all of them decode.
  speed  config 4 (N = 1024, payload 1304, 65 536 frames) and N = 64 (payload 560): HAMMING74_SOFT and CONV_K7 decode, each of its
         own capture of the same payloads, alternated in one process after a warm-up of both; device-event ms per pass.  With
         --kernel-stats (the kernel_stats.csv of a `tools/kstats.sh conv tools/bench_conv.py --speed-only --shapes <one>` run) the
         ms per pass of k_viterbi_k7 and k_conv_encode and trellis steps per second = frames x steps / kernel time.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, bit_errors, capture, link_on, median, save_record  # noqa: E402

MODES = (("hamming74", api.ECC_HAMMING74), ("hamming74_soft", api.ECC_HAMMING74_SOFT), ("conv_k7", api.ECC_CONV_K7))


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


def ber(n, payload, snrs, n_frames, seed):
    ctxs = {name: _ctx(n, ecc) for name, ecc in MODES}
    rows = []
    for snr in snrs:
        row, res, oks = {"snr_db": snr}, {}, {}
        for name, c in ctxs.items():
            if name == "hamming74_soft":   # the frames on the wire are those of hamming74: the same capture
                rx = res["hamming74"][1]
            else:
                pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            r = c.decode_batch(rx, max_symbols=c.data_symbols(payload))
            want = payload if name == "conv_k7" else (payload + 3) // 4 * 4
            oks[name] = (r["status"] == 0) & (r["len"] == want)
            res[name] = (r, rx, pay)
        every = oks["hamming74"] & oks["hamming74_soft"] & oks["conv_k7"]
        some = oks["hamming74"] | oks["hamming74_soft"] | oks["conv_k7"]
        row["frames_compared"] = int(every.sum())
        row["header_mismatches"] = int((some & ~every).sum())
        row["frames_ok"] = {name: int(ok.sum()) for name, ok in oks.items()}
        for name in ctxs:
            r, _, pay = res[name]
            diff = torch.bitwise_xor(r["bytes"][:, :payload], pay)[every]
            bits = bit_errors(diff)
            row[name] = {"payload_bit_errors": bits, "ber": bits / max(1, row["frames_compared"] * payload * 8),
                         "frames_with_errors": int((diff != 0).any(dim=1).sum())}
        rows.append(row)
        del res, rx
        torch.cuda.empty_cache()
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample", "points": rows}


def speed(n, n_frames, payload, reps):
    s, v = _ctx(n, api.ECC_HAMMING74_SOFT), _ctx(n, api.ECC_CONV_K7)
    g = torch.Generator(device=s.device); g.manual_seed(4)
    pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=s.device, generator=g)
    res = {"n_fft": n, "frames": n_frames, "payload": payload}
    caps = {}
    for name, c in (("hamming74_soft", s), ("conv_k7", v)):
        D = c.data_symbols(payload)
        caps[name] = (c, capture(c, g, n_frames, pay, c.frame_samples(payload) + 256, 4_000_003), D)
    # warm-up of both, then alternated: soft Hamming, conv, soft Hamming, conv ...
    times = alternated_ms({name: (c, lambda c=c, x=x, D=D: c.decode_batch(x, max_symbols=D)) for name, (c, x, D) in caps.items()}, reps)
    for name, (c, x, D) in caps.items():
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        m = median(times[name])
        ok = (r["status"] == 0) & (r["len"] >= payload)
        res[name] = {"ms_per_pass": m, "ms_all": times[name], "data_symbols": D, "coded_len": c.coded_len(payload),
                     "slot_bytes": n_frames * x.shape[1] * 8, "dispatch": c.last_dispatch(),
                     "frames_exact": int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())}
    res["trellis_steps_per_frame"] = 4 * v.coded_len(payload)
    res["conv_over_soft_hamming"] = res["conv_k7"]["ms_per_pass"] / res["hamming74_soft"]["ms_per_pass"]
    v.timer_start(); v.encode_batch(pay[:8192].contiguous()); res["conv_k7"]["encode_8192_frames_ms"] = v.timer_stop_ms()
    res["conv_k7"]["encode_dispatch"] = v.last_dispatch()
    del caps
    torch.cuda.empty_cache()
    return res


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return out


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
    ap.add_argument("--shapes", default="cfg4,n64", help="speed blocks to run (one per process for an unambiguous kernel_stats.csv)")
    ap.add_argument("--kernel-stats", default=None, help="cfg4=path,n64=path: kernel_stats.csv of a --speed-only --shapes <one> run each")
    ap.add_argument("--resources", default=None, help="JSON file with the compiler's resource figures of the two kernels, copied into the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_conv.py", "llr_scale": api.SOFT_LLR_SCALE, "device": torch.cuda.get_device_name(0)}
    if not a.ber_only:
        shapes = {"cfg4": lambda: speed(1024, a.cfg4_frames, 1304, a.reps), "n64": lambda: speed(64, a.n64_frames, 560, a.reps)}
        rec["speed"] = {k: shapes[k]() for k in a.shapes.split(",")}
        stats = dict(kv.split("=", 1) for kv in a.kernel_stats.split(",")) if a.kernel_stats else {}
        for shape, path in stats.items():
            blk = rec["speed"].get(shape)
            if blk is None:
                continue
            ks = kernel_stats(path)
            passes = a.reps + 2   # conv decode ran warm-up + reps + the checked pass
            blk["kernel_stats"] = {"source": os.path.basename(path), "conv_decode_passes": passes}
            for kname in ("k_viterbi_k7", "k_conv_encode"):
                hit = [v for k, v in ks.items() if kname in k]
                if hit:
                    blk["kernel_stats"][kname] = {"calls": sum(v["calls"] for v in hit), "total_ms": sum(v["total_ms"] for v in hit)}
            vit = blk["kernel_stats"].get("k_viterbi_k7")
            if vit:
                ms = vit["total_ms"] / passes
                vit["ms_per_pass"] = ms
                vit["trellis_steps_per_second"] = blk["frames"] * blk["trellis_steps_per_frame"] / (ms / 1e3)
    if a.resources:
        rec["kernel_resources"] = json.load(open(a.resources))
    if not a.speed_only:
        rec["ber"] = [ber(64, 560, [float(v) for v in a.snrs.split(",")], a.ber_frames, 11),
                      ber(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.ber_frames, 12)]
    print(json.dumps(rec))
    if not a.speed_only:
        save_record(rec, a.out)


if __name__ == "__main__":
    main()
