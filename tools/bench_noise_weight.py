"""EXT-11 noise-aware LLR weights (ofdm_rx_noise_bins_batch, ofdm_rx_llr_weighted_batch, OFDM_LLRW_NOISE; definition:
tests/noise_weight_ref.py): what the rule wins under a narrow-band interferer, what it costs in a clean channel, and what the mode
costs in time.  Prints one JSON record and writes it to profiles/noise_weight_ber_and_speed.json (--out).  The captures are
tools/link.py's seeded link (link_on) with a complex tone added on top.

  frames    N = 64, 64-QAM, guard bands, --payload bytes, --frames frames a point, for LDPC648, CONV_K7F_R12 and RS255_K7F_R34: frames
            delivered right / delivered wrong (status 0, other bytes) / reported (status != 0), with the mode off against on, ON THE
            SAME CAPTURES.
              tone   14 dB, a tone of power isr_db relative to the frame's own mean power, -20 ... -5 dB, at the fractional bins 11.3
                     and 40.7, over the whole capture
              clean  no tone, 4 ... 9 dB: the rule's cost where every carrier has the same noise
  speed     the decode pass over --speed-frames N = 64 frames (40 dB speed capture of tools/link.py) with the mode off against on,
            alternated in one process, --reps passes each, with spread; and k_noise_bins alone on the pass's own offset / f_delta /
            status arrays."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, capture, generator, link_on, median, open_record  # noqa: E402

N, MOD, SEED = 64, api.QAM64, 11100
MODES = {"LDPC648": api.ECC_LDPC648, "K7F_R12": api.ECC_CONV_K7F_R12, "RS255_K7F_R34": api.ECC_RS255_K7F_R34}


def add_tone(c, rx, frame_samples, isr_db, tone_bin):
    """rx [n_frames, span] with a complex tone at tone_bin on top, isr_db relative to every frame's own mean power (the capture's energy
    over the frame's samples: what lies outside the frame is noise only)"""
    power = rx.abs().pow(2).sum(dim=1).double() / frame_samples
    amp = torch.sqrt(power * 10.0 ** (isr_db / 10.0))
    k = torch.arange(rx.shape[1], device=c.device, dtype=torch.float64)
    tone = torch.exp(2j * math.pi * tone_bin * k / N)
    return (rx + (amp[:, None] * tone[None, :]).to(torch.complex64)).contiguous()


def counts(c, rx, pay, D, exact):
    r = c.decode_batch(rx, max_symbols=D)
    torch.cuda.synchronize()
    ok = r["status"] == 0
    length_ok = (r["len"] == pay.shape[1]) if exact else (r["len"] >= pay.shape[1])
    right = ok & length_ok & (r["bytes"][:, :pay.shape[1]] == pay).all(dim=1)
    return {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum())}


def point(name, ecc, n_frames, payload, snr, isr_db, tone_bin, seed):
    off = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc)
    on = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc, llr_weight=api.LLRW_NOISE)
    pay, rx = link_on(off, n_frames, payload, snr, seed)
    if isr_db is not None:
        rx = add_tone(off, rx, off.frame_samples(payload), isr_db, tone_bin)
    D = off.data_symbols(payload)
    exact = ecc not in (api.ECC_RS255_K7F_R12, api.ECC_RS255_K7F_R23, api.ECC_RS255_K7F_R34)   # RS delivers whole blocks
    row = {"snr_db": snr, "isr_db": isr_db, "tone_bin": tone_bin, "frames": n_frames, "seed": seed,
           "off": counts(off, rx, pay, D, exact), "on": counts(on, rx, pay, D, exact)}
    del rx
    torch.cuda.empty_cache()
    return row


def frames_block(n_frames, payload, isrs, bins, clean_snrs):
    out = {"n_fft": N, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "tone_snr_db": 14.0, "modes": {}}
    for name, ecc in MODES.items():
        tone = [point(name, ecc, n_frames, payload, 14.0, isr, b, SEED + ecc + 100 * i + 10 * j)
                for j, b in enumerate(bins) for i, isr in enumerate(isrs)]
        clean = [point(name, ecc, n_frames, payload, snr, None, None, SEED + ecc + 1000 + i) for i, snr in enumerate(clean_snrs)]
        out["modes"][name] = {"ecc": ecc, "tone": tone, "clean": clean}
    return out


def speed(ecc, n_frames, payload, reps):
    off = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc)
    on = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc, llr_weight=api.LLRW_NOISE)
    D = off.data_symbols(payload)
    g = generator(off, 5)
    pay = torch.randint(0, 256, (n_frames, payload), dtype=torch.uint8, device=off.device, generator=g)
    x = capture(off, g, n_frames, pay, off.frame_samples(payload) + 160, 5_100_003)
    r = off.decode_batch(x, max_symbols=D)
    q = torch.empty((n_frames, N), dtype=torch.float32, device=off.device)

    def kernel():
        rc = off.lib.ofdm_rx_noise_bins_batch(off.h, x.data_ptr(), n_frames, x.shape[1], x.shape[1], r["offset"].data_ptr(),
                                              r["f_delta"].data_ptr(), r["status"].data_ptr(), None, q.data_ptr())
        assert rc == 0

    runs = {"decode_off": (off, lambda: off.decode_batch(x, max_symbols=D)), "decode_on": (on, lambda: on.decode_batch(x, max_symbols=D)),
            "k_noise_bins": (off, kernel)}
    ts = alternated_ms(runs, reps)
    ron = on.decode_batch(x, max_symbols=D)
    torch.cuda.synchronize()
    right = (ron["status"] == 0) & (ron["len"] == payload) & (ron["bytes"][:, :payload] == pay).all(dim=1)
    out = {"n_fft": N, "ecc": ecc, "frames": n_frames, "payload": payload, "data_symbols": D, "dispatch_on": on.last_dispatch(),
           "frames_right_on": int(right.sum())}
    for name in runs:
        out[name] = {"ms_per_pass": median(ts[name]), "ms_all": ts[name], "spread_ms": max(ts[name]) - min(ts[name])}
    out["on_over_off"] = out["decode_on"]["ms_per_pass"] / out["decode_off"]["ms_per_pass"]
    out["k_noise_bins_ns_per_frame"] = 1e6 * out["k_noise_bins"]["ms_per_pass"] / n_frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="frames,speed")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--payload", type=int, default=560)
    ap.add_argument("--isrs", default="-20,-15,-10,-5")
    ap.add_argument("--bins", default="11.3,40.7")
    ap.add_argument("--clean-snrs", default="4,5,6,7,8,9")
    ap.add_argument("--speed-frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_weight_ber_and_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_noise_weight.py", "device": torch.cuda.get_device_name(0),
           "definition": "parity unpinned by the reference: tests/noise_weight_ref.py is the definition"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    if "frames" in blocks:
        rec["frames"] = frames_block(a.frames, a.payload, [float(v) for v in a.isrs.split(",")], [float(v) for v in a.bins.split(",")],
                                     [float(v) for v in a.clean_snrs.split(",")])
        save()
    if "speed" in blocks:
        rec["speed"] = {name: speed(MODES[name], a.speed_frames, a.payload, a.reps) for name in ("LDPC648", "K7F_R12")}
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
