"""EXT-8 wide CFO acquisition (ofdm_cfo_wide_batch, OFDM_CFO_WIDE; definition: tests/cfo_wide_ref.py): how often the training blocks name
the right multiple of 2 pi / S, by what margin, and what the mode costs.  Prints one JSON record and writes it to
profiles/cfo_wide_accuracy_and_speed.json (--out).  Runs on tools/link.py's seeded wide link (wide_link_on: m uniform over +-span, a
fractional part within +-0.95 pi / S).

  accuracy  64-QAM, guard bands, ECC_NONE, --frames frames a point, per snr_db (the channel's; the data symbols see data_snr of it):
            frames Schmidl-Cox detects (status 0 of a CFO_SIGNED decode, whose offset and f_delta the stage is given), the share of
            them with the right m, and the smallest and the median ratio of the winner's window energy to the runner-up's.
            N = 64 from 0 dB, below which Schmidl-Cox detects next to nothing, to 16 dB; N = 1024 at 26 ... 38 dB.
  speed     the decode pass under CFO_WIDE next to the same capture's pass under CFO_SIGNED, and k_cfo_wide alone on the pass's own
            offset / f_delta / status arrays, alternated in one process, --reps passes each, with spread.  The capture is
            tools/link.py's speed capture (40 dB, every offset inside the old range: the kernel's work does not depend on m).
            frames_exact_cfo_wide counts byte-exact uncoded frames and is there to show that the pass decodes: at N = 1024 the data
            symbols of that capture see 28 dB (data_snr), where most uncoded 64-QAM frames of 2000 bytes hold a wrong bit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, capture, data_snr, generator, median, open_record, wide_link_on  # noqa: E402

MOD, SEED = api.QAM64, 8100
PAYLOAD = {64: 100, 1024: 300}


def accuracy_point(n, snr, n_frames, span):
    s = api.Context(n_fft=n, modulation=MOD, guard_bands=True)
    payload = PAYLOAD[n]
    pay, rx, m_true, _ = wide_link_on(s, n_frames, payload, snr, SEED + n + int(round(10 * snr)), span)
    r = s.decode_batch(rx, max_symbols=s.data_symbols(payload))
    w = s.cfo_wide(rx, r["offset"], r["f_delta"], span, status=r["status"])
    torch.cuda.synchronize()
    found = (r["status"] == 0) & (w["metric"][:, 0] > 0)          # detected, and the training blocks inside the capture
    row = {"snr_db": snr, "data_snr_db": float(data_snr(n, snr)), "frames": n_frames, "detected": int(found.sum())}
    if row["detected"]:
        ratio = (w["metric"][:, 0] / w["metric"][:, 1])[found].double()
        right = (w["m"] == m_true)[found]
        row.update({"right": int(right.sum()), "share_right": float(right.double().mean()), "ratio_min": float(ratio.min()),
                    "ratio_median": float(ratio.median()), "ratio_min_among_right": float(ratio[right].min()) if bool(right.any()) else None})
    return row


def accuracy(n, snrs, n_frames, span):
    out = {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "ecc": "NONE", "payload": PAYLOAD[n], "span": span,
           "seed": "SEED + n_fft + 10 snr_db", "points": []}
    for snr in snrs:
        out["points"].append(accuracy_point(n, snr, n_frames, span))
        torch.cuda.empty_cache()
    return out


def speed(n, n_frames, payload, reps):
    w = api.Context(n_fft=n, modulation=MOD, guard_bands=True, cfo_mode=api.CFO_WIDE)
    s = api.Context(n_fft=n, modulation=MOD, guard_bands=True, cfo_mode=api.CFO_SIGNED)
    D = s.data_symbols(payload)
    g = generator(s, 5)
    pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=s.device, generator=g)
    x = capture(s, g, n_frames, pay, s.frame_samples(payload) + 160, 5_100_003)
    r = s.decode_batch(x, max_symbols=D)
    fd = r["f_delta"].clone()
    m = torch.empty((n_frames,), dtype=torch.int32, device=s.device)
    metric = torch.empty((n_frames, 2), dtype=torch.float32, device=s.device)

    def kernel():
        rc = s.lib.ofdm_cfo_wide_batch(s.h, x.data_ptr(), n_frames, x.shape[1], x.shape[1], r["offset"].data_ptr(), r["status"].data_ptr(),
                                       api.CFO_WIDE_SPAN, fd.data_ptr(), m.data_ptr(), metric.data_ptr())
        assert rc == 0

    runs = {"decode_cfo_wide": (w, lambda: w.decode_batch(x, max_symbols=D)), "decode_cfo_signed": (s, lambda: s.decode_batch(x, max_symbols=D)),
            "k_cfo_wide": (s, kernel)}
    ts = alternated_ms(runs, reps)
    rw = w.decode_batch(x, max_symbols=D)
    torch.cuda.synchronize()
    right = (rw["status"] == 0) & (rw["len"] == payload) & (rw["bytes"][:, :payload] == pay).all(dim=1)
    out = {"n_fft": n, "frames": n_frames, "payload": payload, "data_symbols": D, "span": api.CFO_WIDE_SPAN, "dispatch": w.last_dispatch(),
           "frames_exact_cfo_wide": int(right.sum()), "same_f_delta_as_signed": bool(torch.equal(rw["f_delta"], r["f_delta"]))}
    for name in runs:
        out[name] = {"ms_per_pass": median(ts[name]), "ms_all": ts[name], "spread_ms": max(ts[name]) - min(ts[name])}
    out["wide_over_signed"] = out["decode_cfo_wide"]["ms_per_pass"] / out["decode_cfo_signed"]["ms_per_pass"]
    out["k_cfo_wide_ns_per_frame"] = 1e6 * out["k_cfo_wide"]["ms_per_pass"] / n_frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="accuracy64,accuracy1024,speed64,speed1024")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--snrs64", default="0,2,4,6,8,10,12,14,16")
    ap.add_argument("--snrs1024", default="26,28,30,32,34,36,38")
    ap.add_argument("--span", type=int, default=api.CFO_WIDE_SPAN)
    ap.add_argument("--speed-frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfo_wide_accuracy_and_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_cfo_wide.py", "device": torch.cuda.get_device_name(0),
           "definition": "parity unpinned by the reference: tests/cfo_wide_ref.py is the definition"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    for n, snrs in ((64, a.snrs64), (1024, a.snrs1024)):
        if f"accuracy{n}" in blocks:
            rec[f"accuracy{n}"] = accuracy(n, [float(v) for v in snrs.split(",")], a.frames, a.span)
            save()
    if "speed64" in blocks:
        rec["speed64"] = speed(64, a.speed_frames, 560, a.reps)
        save()
    if "speed1024" in blocks:
        rec["speed1024"] = speed(1024, max(a.speed_frames // 16, 1), 2000, a.reps)
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
