"""Soft-decision receive (OFDM_ECC_HAMMING74_SOFT) against hard Hamming(7,4) decoding: speed and BER.  Prints one JSON record and
writes it to profiles/soft_ber_and_speed.json (--out).

  speed  config 4 (N = 1024, 64-QAM, guard bands, Hamming, the 65 536-frame capture of tools/bench_large_n.py) and the same at N = 64
         (payload 560 B): hard and soft decode of the same capture alternated in one process, ms per pass, the fraction of 8 TB/s on one
         read of the slot bytes; with --kernel-stats (the kernel_stats.csv of a `tools/kstats.sh soft tools/bench_soft.py --speed-only`
         run) per-kernel ms per pass, and for k_sym<llr> / k_rx_finish_soft the fraction of 8 TB/s on the bytes each must move.
  ber    N = 64 and N = 1024, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32, CFO), a seeded SNR grid:
         payload bit errors of both decoders over the frames both report FRAME_OK with the true length, frames compared, header
         mismatches (frames where exactly one of the two reports FRAME_OK and the true length).
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
from tools.link import alternated_ms, bit_errors, link_on, median, save_record  # noqa: E402

HBM_PEAK = 8.0e12


def _ctxs(n):
    return (api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_HAMMING74),
            api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=api.ECC_HAMMING74_SOFT))


def speed(n, n_frames, payload, reps):
    from tools.bench_large_n import _cfg4_ring

    h, s = _ctxs(n)
    g = torch.Generator(device=h.device); g.manual_seed(4)
    D, flen = h.data_symbols(payload), h.frame_samples(payload)
    span = flen + 256
    if n == 1024 and payload == 1304:
        x, pay = _cfg4_ring(h, g, n_frames, span, 40.0, 0)
    else:
        pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=h.device, generator=g)
        tx = h.encode_batch(pay)
        d = torch.randint(1, 65, (n_frames,), dtype=torch.int32, device=h.device, generator=g)
        x = h.channel_batch(tx, snr_db=40.0, seed=4, delay=d, span=span)
        del tx
    slot = n_frames * span * 8
    res = {"n_fft": n, "frames": n_frames, "payload": payload, "data_symbols": D, "slot_bytes": slot}
    times = alternated_ms({"hard": (h, lambda: h.decode_batch(x, max_symbols=D)), "soft": (s, lambda: s.decode_batch(x, max_symbols=D))}, reps)
    rh, rs = h.decode_batch(x, max_symbols=D), s.decode_batch(x, max_symbols=D)
    torch.cuda.synchronize()
    for name, ms, r, c in (("hard", times["hard"], rh, h), ("soft", times["soft"], rs, s)):
        m = median(ms)
        ok = (r["status"] == 0) & (r["len"] >= payload)
        res[name] = {"ms_per_pass": m, "ms_all": ms, "of_8tbs_on_slot_bytes": slot / (m / 1e3) / HBM_PEAK, "dispatch": c.last_dispatch(),
                     "frames_exact": int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())}
    res["soft_over_hard"] = res["soft"]["ms_per_pass"] / res["hard"]["ms_per_pass"]
    nd, bps = s.data_carriers, s.modulation
    coded = s.coded_len(payload)
    # bytes each soft kernel must move per frame: k_sym<llr> reads the data symbols (CP skipped) and H, writes LLRs and hard bytes;
    # k_rx_finish_soft reads the header, the body's LLRs, writes the payload
    res["required_bytes_per_frame"] = {"k_sym<llr>": D * n * 8 + n * 8 + D * nd * bps + D * nd * bps // 8,
                                       "k_rx_finish_soft": 16 + coded // 7 * 56 + coded // 7 * 4}
    del x
    torch.cuda.empty_cache()
    return res


def ber(n, payload, snrs, n_frames, seed, scales=()):
    h, s = _ctxs(n)
    D = h.data_symbols(payload)
    rows = []
    for snr in snrs:
        pay, rx = link_on(h, n_frames, payload, snr, seed + int(10 * snr))
        want = (payload + 3) // 4 * 4
        row = {"snr_db": snr}
        oks = []
        for name, c in (("hard", h), ("soft", s)):
            r = c.decode_batch(rx, max_symbols=D)
            oks.append((r["status"] == 0) & (r["len"] == want))
            row[name] = r
        row["_soft_raw"] = row["soft"]
        both = oks[0] & oks[1]
        row["frames_compared"] = int(both.sum())
        row["header_mismatches"] = int((oks[0] ^ oks[1]).sum())
        for name in ("hard", "soft"):
            diff = torch.bitwise_xor(row[name]["bytes"][:, :payload], pay)[both]
            bits = bit_errors(diff)
            row[name] = {"payload_bit_errors": bits, "ber": bits / max(1, row["frames_compared"] * payload * 8),
                         "frames_with_errors": int((diff != 0).any(dim=1).sum())}
        if scales:   # the same decode through the stages (rx_llr + hamming74_decode_soft) at other LLR scales
            r = row.pop("_soft_raw")
            hk = s.estimate_channel(rx, r["offset"], r["f_delta"])
            nb = (payload + 3) // 4   # 7-byte code blocks = 56 LLRs each
            row["payload_bit_errors_by_scale"] = {}
            for sc in scales:
                L = s.rx_llr(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk, scale=sc)
                dec = s.hamming74_decode_soft(L[:, 128:128 + nb * 56].contiguous()).view(n_frames, -1)[:, :payload]
                diff = torch.bitwise_xor(dec, pay)[both]
                row["payload_bit_errors_by_scale"][str(sc)] = bit_errors(diff)
        row.pop("_soft_raw", None)
        rows.append(row)
        del rx
    torch.cuda.empty_cache()
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample", "points": rows}


def kernel_stats(path, passes):
    """per-kernel ms per pass from a kernel_stats.csv of the --speed-only run (each shape decoded `passes` times per decoder)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            out[name] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
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
    ap.add_argument("--snrs-1024", default="22,24,26,28,30,32,34,36,38,40",
                    help="N = 1024 grid: there the header blocks dominate the pseudo-variance the channel scales its noise by, so the data "
                         "symbols see ~12 dB less (tools/bench_large_n.py)")
    ap.add_argument("--shapes", default="cfg4,n64", help="speed blocks to run (one per process for an unambiguous kernel_stats.csv)")
    ap.add_argument("--kernel-stats", default=None, help="cfg4=path,n64=path: kernel_stats.csv of a --speed-only --shapes <one> run each")
    ap.add_argument("--scales", default="4,8,16,32,64", help="N = 64 BER points: the soft decode again at these LLR scales (stages)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_ber_and_speed.json"))
    a = ap.parse_args()
    rec = {"tool": "tools/bench_soft.py", "llr_scale": api.SOFT_LLR_SCALE, "device": torch.cuda.get_device_name(0)}
    if not a.ber_only:
        shapes = {"cfg4": lambda: speed(1024, a.cfg4_frames, 1304, a.reps), "n64": lambda: speed(64, a.n64_frames, 560, a.reps)}
        rec["speed"] = {k: shapes[k]() for k in a.shapes.split(",")}
        stats = dict(kv.split("=", 1) for kv in a.kernel_stats.split(",")) if a.kernel_stats else {}
        for shape, path in stats.items():
            blk = rec["speed"].get(shape)
            if blk is None:
                continue
            ks = kernel_stats(path, a.reps + 2)   # each decoder ran warm-up + reps + the checked pass
            blk["kernel_stats"] = {"source": os.path.basename(path), "passes_per_decoder": a.reps + 2,
                                   "ms_per_pass": {k: v["total_ms"] / (a.reps + 2) for k, v in ks.items()}}
            n = blk["n_fft"]
            for kname, key in ((f"k_sym<{n}, 6>", "k_sym<llr>"), ("k_rx_finish_soft", "k_rx_finish_soft")):
                hit = [v for k, v in ks.items() if kname in k]
                if hit:
                    ms = sum(v["total_ms"] for v in hit) / (a.reps + 2)
                    need = blk["required_bytes_per_frame"][key] * blk["frames"]
                    blk.setdefault("kernels", {})[key] = {"ms_per_pass": ms, "of_8tbs_on_required_bytes": need / (ms / 1e3) / HBM_PEAK}
    if not a.speed_only:
        snrs = [float(v) for v in a.snrs.split(",")]
        scales = [float(v) for v in a.scales.split(",") if v]
        rec["ber"] = [ber(64, 560, snrs, a.ber_frames, 11, scales), ber(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.ber_frames, 12)]
    print(json.dumps(rec))
    if not a.speed_only:
        save_record(rec, a.out)


if __name__ == "__main__":
    main()
