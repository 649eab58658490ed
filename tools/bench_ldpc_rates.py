"""OFDM_ECC_LDPC648_R23 / _R34 / _R56 next to OFDM_ECC_LDPC648, OFDM_ECC_CONV_K7F_R23 and _R34: frames right / wrong / reported, air time
and speed.  Prints one JSON record and writes it to profiles/ldpc_rates_ber_and_speed.json (--out).  The modes are parity unpinned by
the reference: tests/ldpc_rates_ref.py is the definition.

  ber      N = 64 at 4 .. 18 dB and N = 1024 at 26 .. 40 dB, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32,
           CFO): the same payloads, delays, CFO and channel seed for the six modes, every mode encoded by its own context.  Per point
           and mode: right (status 0, the true length and the true bytes), wrong (status 0 otherwise), reported (any other status).
  point    the link tests/test_gpu_ldpc_rates.py runs (tools/link.py; 256 frames, seed 9012) for K7F_R34 and LDPC648_R34 at the highest
           point of the N = 64 sweep at which K7F_R34 delivers fewer than 90 % of its frames whole, and at its two neighbours.
  kernel   k_ldpc_decode<r23|r34|r56> and k_ldpc_decode alone (Context.ldpc_decode) on rows of 10 code words, alternated in one process:
           clean LLRs (+-32) and the LLRs of each mode's own N = 64 link at the middle of the sweep, max_iter 20: ms, ns per code
           word, mean iterations of the converged code words, share unconverged.
  speed    65 536 N = 64 frames (payload 560): the decode pass of each new mode alternated with LDPC648's in one process after a warm-up
           of all, --reps passes each; device-event ms per pass and the spread of every mode's passes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, delivered, link, link_on, median, open_record  # noqa: E402

LDPC = (("ldpc648", api.ECC_LDPC648, 0), ("ldpc648_r23", api.ECC_LDPC648_R23, 1), ("ldpc648_r34", api.ECC_LDPC648_R34, 2),
        ("ldpc648_r56", api.ECC_LDPC648_R56, 3))
MODES = tuple((n, e) for n, e, _ in LDPC) + (("k7f_r23", api.ECC_CONV_K7F_R23), ("k7f_r34", api.ECC_CONV_K7F_R34))


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


def _counts(r, pay, payload):
    right, ok = delivered(r, pay, payload)
    return {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum())}


def ber(n, payload, snrs, n_frames, seed):
    ctxs = {name: _ctx(n, ecc) for name, ecc in MODES}
    rows = []
    for snr in snrs:
        row = {"snr_db": snr}
        for name, c in ctxs.items():
            pay, rx = link_on(c, n_frames, payload, snr, seed + int(10 * snr))
            r = c.decode_batch(rx, max_symbols=c.data_symbols(payload))
            torch.cuda.synchronize()
            del rx
            row[name] = _counts(r, pay, payload)
            row[name]["status_counts"] = {str(int(s)): int((r["status"] == s).sum()) for s in torch.unique(r["status"]).tolist()}
        rows.append(row)
        torch.cuda.empty_cache()
    air = {name: {"coded_len": c.coded_len(payload), "data_symbols": c.data_symbols(payload), "frame_samples": c.frame_samples(payload)}
           for name, c in ctxs.items()}
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample",
            "caveat": "frames of different length see slightly different noise at equal snr_db (the noise is scaled by the whole frame's "
                      "pseudo-variance)", "air_time": air, "points": rows}


def point_snr(rec):
    """the highest point of the N = 64 sweep at which K7F_R34 delivers fewer than 90 % of its frames whole"""
    sweep = rec["ber"][0]
    return max(p["snr_db"] for p in sweep["points"] if p["k7f_r34"]["right"] < 0.9 * sweep["frames_per_point"])


def point(rec, n_frames=256, payload=560, seed=9012):
    """the counts of tests/test_gpu_ldpc_rates.py::test_ldpc_r34_against_the_framed_viterbi_r34_on_one_link over the link that test runs,
    and at the neighbouring points of the sweep"""
    snr = point_snr(rec)
    out = {"snr_db": snr, "frames": n_frames, "payload": payload, "seed": seed, "points": []}
    for s in (snr - 1.0, snr, snr + 1.0):
        row = {"snr_db": s}
        for name, ecc in (("k7f_r34", api.ECC_CONV_K7F_R34), ("ldpc648_r34", api.ECC_LDPC648_R34)):
            c, pay, rx, D = link(ecc, 64, api.QAM64, n_frames, payload, s, seed)
            r = c.decode_batch(rx, max_symbols=D)
            torch.cuda.synchronize()
            row[name] = _counts(r, pay, payload)
        out["points"].append(row)
    return out


def _noisy_llrs(ecc, k, n_frames, n_cw, snr):
    """the LLRs the N = 64 link hands the mode's decode kernel at `snr`, rows of n_cw code words"""
    c = _ctx(64, ecc)
    payload = k * n_cw - 8
    pay, rx = link_on(c, n_frames, payload, snr, 77)
    D = c.data_symbols(payload)
    r = c.decode_batch(rx, max_symbols=D)
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    L = c.rx_llr(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
    keep = r["status"] != api.FRAME_NOSYNC
    return c, L[keep][:, 128:128 + 640 * n_cw].contiguous()


def kernel_alone(n_frames, n_cw, snr, reps, max_iter=20):
    sets = {}
    for name, ecc, rate in LDPC:
        k = api.LDPC_INFO_BYTES[rate]
        c, noisy = _noisy_llrs(ecc, k, n_frames, n_cw, snr)
        g = torch.Generator(device=c.device); g.manual_seed(5)
        info = torch.randint(0, 256, (noisy.shape[0], k * n_cw), dtype=torch.uint8, device=c.device, generator=g)
        code = c.ldpc_encode(info, rate=rate)
        bits = (code[:, :, None] >> torch.arange(8, device=c.device, dtype=torch.uint8)) & 1
        clean = (bits.reshape(code.shape[0], -1).to(torch.int8) * 64 - 32).contiguous()
        by, it = c.ldpc_decode(clean, max_iter=max_iter, rate=rate)
        assert torch.equal(by, info) and bool((it == 1).all())
        sets[name] = (c, rate, clean, noisy)
    out = {"frames": n_frames, "codewords_per_frame": n_cw, "noisy_snr_db": snr, "max_iter": max_iter, "runs": []}
    for which in (2, 3):
        runs = {name: (v[0], lambda v=v: v[0].ldpc_decode(v[which], max_iter=max_iter, rate=v[1])) for name, v in sets.items()}
        ts = alternated_ms(runs, reps)
        for name, v in sets.items():
            by, it = v[0].ldpc_decode(v[which], max_iter=max_iter, rate=v[1])
            conv = it > 0
            ms = median(ts[name])
            out["runs"].append({"kernel": v[0].last_dispatch(), "llrs": "clean" if which == 2 else "noisy", "ms": ms, "ms_all": ts[name],
                                "codewords": int(it.numel()), "ns_per_codeword": ms * 1e6 / it.numel(), "unconverged": int((~conv).sum()),
                                "mean_iterations_converged": float(it[conv].float().mean()) if conv.any() else None,
                                "iterations_run": int(torch.where(conv, it, torch.full_like(it, max_iter)).sum())})
    return out


def speed(n, n_frames, payload, reps):
    res = {"n_fft": n, "frames": n_frames, "payload": payload}
    caps = {}
    for name, ecc, _ in LDPC:
        c = _ctx(n, ecc)
        x = torch.empty((n_frames, c.frame_samples(payload) + 160), dtype=torch.complex64, device=c.device)
        pays = []
        for lo in range(0, n_frames, 8192):
            hi = min(lo + 8192, n_frames)
            pay, rx = link_on(c, hi - lo, payload, 40.0, 4_000_003 + lo)
            x[lo:hi] = rx
            pays.append(pay)
            del rx
        caps[name] = (c, x, c.data_symbols(payload), torch.cat(pays))
    times = alternated_ms({name: (c, lambda c=c, x=x, D=D: c.decode_batch(x, max_symbols=D)) for name, (c, x, D, _) in caps.items()}, reps)
    for name, (c, x, D, pay) in caps.items():
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        right, _ = delivered(r, pay, payload)
        res[name] = {"ms_per_pass": median(times[name]), "ms_all": times[name], "spread_ms": max(times[name]) - min(times[name]),
                     "data_symbols": D, "coded_len": c.coded_len(payload), "frame_samples": c.frame_samples(payload),
                     "dispatch": c.last_dispatch(), "frames_exact": int(right.sum())}
    for name, _, _ in LDPC[1:]:
        res[name + "_over_ldpc648"] = res[name]["ms_per_pass"] / res["ldpc648"]["ms_per_pass"]
    del caps
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="ber,point,kernel,speed,ber1024", help="which of ber, point, kernel, speed, ber1024 to run")
    ap.add_argument("--n64-frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ber-frames", type=int, default=4096)
    ap.add_argument("--snrs", default="4,5,6,7,8,9,10,11,12,13,14,15,16,17,18", help="N = 64 grid (dB, channel.rs definition)")
    ap.add_argument("--snrs-1024", default="26,28,30,32,34,36,38,40", help="N = 1024 grid")
    ap.add_argument("--kernel-frames", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpc_rates_ber_and_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_ldpc_rates.py", "llr_scale": api.SOFT_LLR_SCALE, "ldpc_max_iter": api.LDPC_MAX_ITER,
           "device": torch.cuda.get_device_name(0),
           "definition": "parity unpinned by the reference: tests/ldpc_rates_ref.py is the definition"}
    # blocks measured by an earlier call stay; saved after every block: a later block that fails does not take the earlier ones with it
    rec, save = open_record(rec, a.out, keep_earlier=True)

    if "ber" in blocks:
        rec["ber"] = [ber(64, 560, [float(v) for v in a.snrs.split(",")], a.ber_frames, 11)] + rec.get("ber", [])[1:]
        save()
    if "point" in blocks:   # needs the sweep, of this call or of an earlier one
        rec["point"] = point(rec)
        save()
    if "kernel" in blocks:
        snrs = [float(v) for v in a.snrs.split(",")]
        rec["kernel"] = kernel_alone(a.kernel_frames, 10, snrs[len(snrs) // 2], a.reps)
        save()
    if "speed" in blocks:
        rec["speed"] = {"n64": speed(64, a.n64_frames, 560, a.reps)}
        save()
    if "ber1024" in blocks:  # behind the N = 64 sweep, of this call or of an earlier one
        rec["ber"] = rec["ber"][:1] + [ber(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.ber_frames, 12)]
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
