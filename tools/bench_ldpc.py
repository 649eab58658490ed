"""OFDM_ECC_LDPC648 next to OFDM_ECC_CONV_K7F_R12 and OFDM_ECC_RS255_K7F_R34: frames right / wrong / reported, air time and speed.
Prints one JSON record and writes it to profiles/ldpc_ber_and_speed.json (--out).  The mode is parity unpinned by the reference:
tests/ldpc_ref.py is the definition.

  ber      N = 64 at 4 .. 16 dB and N = 1024 at 26 .. 38 dB, 64-QAM, guard bands, through ofdm_channel_batch (FIR CHANNEL, delay 1..32,
           CFO): the same payloads, delays, CFO and channel seed for the three modes, every mode encoded by its own context.  Per point
           and mode: right (status 0, the true length and the true bytes), wrong (status 0 otherwise), reported (any other status).
  speed    262 144 N = 64 frames (payload 560) and 65 536 config-4 frames (N = 1024, payload 1304): the decode pass of the three modes,
           each on its own capture of the same payloads, alternated in one process after a warm-up of all, --reps passes each;
           device-event ms per pass and the spread of every mode's passes.
  kernel   k_ldpc_decode alone (Context.ldpc_decode) on rows of 15 code words, clean LLRs (+-32) and the LLRs of the N = 64 link at the
           middle of its sweep, max_iter 5, 10, 20 and 40: ms, average iterations of the converged code words, share unconverged, edge
           updates per second (88 x 27 edges per code word and iteration run).
  point    the link tests/test_gpu_ldpc.py runs (tools/link.py; 1 024 frames, seed 9012) at the highest point of the N = 64 sweep at which K7F_R12
           delivers fewer than 90 % of its frames whole: right / wrong / reported of K7F_R12 and LDPC648.
  host     ofdm_ldpc648_decode on 16 threads over the same noisy rows at max_iter 20, outputs compared with the device's.
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
from tools.link import alternated_ms, delivered, link, link_on, median, open_record  # noqa: E402

MODES = (("k7f_r12", api.ECC_CONV_K7F_R12), ("rs255_k7f_r34", api.ECC_RS255_K7F_R34), ("ldpc648", api.ECC_LDPC648))
EDGES = 88 * 27


def _ctx(n, ecc):
    return api.Context(n_fft=n, modulation=api.QAM64, guard_bands=True, ecc=ecc)


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
            # RS modes deliver whole 223-byte blocks: the payload is their prefix
            right, ok = delivered(r, pay, payload, exact=name != "rs255_k7f_r34")
            row[name] = {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum()),
                         "status_counts": {str(int(s)): int((r["status"] == s).sum()) for s in torch.unique(r["status"]).tolist()}}
        rows.append(row)
        torch.cuda.empty_cache()
    air = {}
    for name, c in ctxs.items():
        air[name] = {"coded_len": c.coded_len(payload), "data_symbols": c.data_symbols(payload), "frame_samples": c.frame_samples(payload)}
    return {"n_fft": n, "modulation": "64-QAM", "guard_bands": True, "payload": payload, "frames_per_point": n_frames, "seed": seed,
            "channel": "ofdm_channel_batch: FIR CHANNEL, delay 1..32, CFO uniform in +-1/S rad/sample",
            "caveat": "frames of different length see slightly different noise at equal snr_db (the noise is scaled by the whole frame's "
                      "pseudo-variance)", "air_time": air, "points": rows}


def speed(n, n_frames, payload, reps):
    res = {"n_fft": n, "frames": n_frames, "payload": payload}
    caps = {}
    for name, ecc in MODES:
        c = _ctx(n, ecc)
        x = torch.empty((n_frames, c.frame_samples(payload) + 160), dtype=torch.complex64, device=c.device)
        pays = []
        for lo in range(0, n_frames, 8192):
            hi = min(lo + 8192, n_frames)
            pay, rx = link_on(c, hi - lo, payload, 40.0, 4_000_003 + lo)
            x[lo:hi] = rx
            pays.append(pay)
            del rx
        D = c.data_symbols(payload)
        caps[name] = (c, x, D, torch.cat(pays))
    # warm-up of all, then alternated
    times = alternated_ms({name: (c, lambda c=c, x=x, D=D: c.decode_batch(x, max_symbols=D)) for name, (c, x, D, _) in caps.items()}, reps)
    for name, (c, x, D, pay) in caps.items():
        r = c.decode_batch(x, max_symbols=D)
        torch.cuda.synchronize()
        ok = (r["status"] == 0) & (r["len"] >= payload)
        res[name] = {"ms_per_pass": median(times[name]), "ms_all": times[name],
                     "spread_ms": max(times[name]) - min(times[name]), "data_symbols": D, "coded_len": c.coded_len(payload),
                     "frame_samples": c.frame_samples(payload), "dispatch": c.last_dispatch(),
                     "frames_exact": int(((r["bytes"][:, :payload] == pay).all(dim=1) & ok).sum())}
    res["ldpc648_over_k7f_r12"] = res["ldpc648"]["ms_per_pass"] / res["k7f_r12"]["ms_per_pass"]
    del caps
    torch.cuda.empty_cache()
    return res


def _noisy_llrs(n_frames, n_cw, snr):
    """the LLRs the N = 64 link hands k_ldpc_decode at `snr`, rows of n_cw code words"""
    c = _ctx(64, api.ECC_LDPC648)
    payload = 40 * n_cw - 8
    pay, rx = link_on(c, n_frames, payload, snr, 77)
    D = c.data_symbols(payload)
    r = c.decode_batch(rx, max_symbols=D)
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    L = c.rx_llr(rx, D, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
    keep = r["status"] != api.FRAME_NOSYNC
    return c, L[keep][:, 128:128 + 640 * n_cw].contiguous()


def kernel_alone(n_frames, n_cw, snr, reps):
    c, noisy = _noisy_llrs(n_frames, n_cw, snr)
    g = torch.Generator(device=c.device); g.manual_seed(5)
    info = torch.randint(0, 256, (noisy.shape[0], 40 * n_cw), dtype=torch.uint8, device=c.device, generator=g)
    code = c.ldpc_encode(info)
    bits = (code[:, :, None] >> torch.arange(8, device=c.device, dtype=torch.uint8)) & 1
    clean = (bits.reshape(code.shape[0], -1).to(torch.int8) * 64 - 32).contiguous()
    out = {"frames": int(noisy.shape[0]), "codewords_per_frame": n_cw, "noisy_snr_db": snr, "runs": []}
    for name, llr in (("clean", clean), ("noisy", noisy)):
        for max_iter in (5, 10, 20, 40):
            ts = alternated_ms({"decode": (c, lambda: c.ldpc_decode(llr, max_iter=max_iter))}, reps)["decode"]
            by, it = c.ldpc_decode(llr, max_iter=max_iter)
            ms = median(ts)
            run = torch.where(it > 0, it, torch.full_like(it, max_iter)).sum().item()
            conv = it > 0
            out["runs"].append({"llrs": name, "max_iter": max_iter, "ms": ms, "ms_all": ts, "codewords": int(it.numel()),
                                "unconverged": int((~conv).sum()), "mean_iterations_converged": float(it[conv].float().mean()) if conv.any() else None,
                                "iterations_run": int(run), "edge_updates_per_s": run * EDGES / (ms * 1e-3)})
            if name == "clean":
                assert torch.equal(by, info) and bool((it == 1).all())
    # the host decoder on 16 threads over the same noisy rows
    lib = c.lib
    h = noisy.cpu().numpy().reshape(-1, 640)
    res = np.zeros((h.shape[0], 40), np.uint8)
    its = np.zeros(h.shape[0], np.int32)
    cuts = np.linspace(0, h.shape[0], 17).astype(int)

    def work(i):
        lo, hi = int(cuts[i]), int(cuts[i + 1])
        if hi > lo:
            lib.ofdm_ldpc648_decode(C.c_void_p(h[lo:hi].ctypes.data), hi - lo, 20, C.c_void_p(res[lo:hi].ctypes.data), C.c_void_p(its[lo:hi].ctypes.data))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(work, range(16)))
    host_s = time.perf_counter() - t0
    by, it = c.ldpc_decode(noisy, max_iter=20)
    out["host_16_threads"] = {"max_iter": 20, "seconds": host_s, "codewords": int(h.shape[0]),
                              "bytes_equal_device": bool((by.cpu().numpy().reshape(-1, 40) == res).all()),
                              "iters_equal_device": bool((it.cpu().numpy().reshape(-1) == its).all())}
    return out


def point(rec, n_frames=1024, payload=560, seed=9012):
    """the counts of tests/test_gpu_ldpc.py::test_ldpc_against_the_framed_viterbi_mode_on_one_link over the link that test runs
    (tools/link.py), at the highest point of the N = 64 sweep at which K7F_R12 delivers fewer than 90 % of its frames whole"""
    sweep = rec["ber"][0]
    below = [p["snr_db"] for p in sweep["points"] if p["k7f_r12"]["right"] < 0.9 * sweep["frames_per_point"]]
    snr = max(below)
    out = {"snr_db": snr, "frames": n_frames, "payload": payload, "seed": seed}
    for name, ecc in (("k7f_r12", api.ECC_CONV_K7F_R12), ("ldpc648", api.ECC_LDPC648)):
        c, pay, rx, D = link(ecc, 64, api.QAM64, n_frames, payload, snr, seed)
        r = c.decode_batch(rx, max_symbols=D)
        torch.cuda.synchronize()
        right, ok = delivered(r, pay, payload)
        out[name] = {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="ber,point,kernel,speed", help="which of ber, point, kernel, speed to run")
    ap.add_argument("--cfg4-frames", type=int, default=65536)
    ap.add_argument("--n64-frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ber-frames", type=int, default=4096)
    ap.add_argument("--snrs", default="4,5,6,7,8,9,10,11,12,13,14,15,16", help="N = 64 grid (dB, channel.rs definition)")
    ap.add_argument("--snrs-1024", default="26,28,30,32,34,36,38", help="N = 1024 grid")
    ap.add_argument("--kernel-frames", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpc_ber_and_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_ldpc.py", "llr_scale": api.SOFT_LLR_SCALE, "ldpc_max_iter": api.LDPC_MAX_ITER,
           "device": torch.cuda.get_device_name(0), "definition": "parity unpinned by the reference: tests/ldpc_ref.py is the definition"}
    # blocks measured by an earlier call stay; saved after every block: a later block that fails does not take the earlier ones with it
    rec, save = open_record(rec, a.out, keep_earlier=True)

    if "ber" in blocks:
        rec["ber"] = [ber(64, 560, [float(v) for v in a.snrs.split(",")], a.ber_frames, 11),
                      ber(1024, 1304, [float(v) for v in a.snrs_1024.split(",")], a.ber_frames, 12)]
        save()
    if "point" in blocks:   # needs the sweep, of this call or of an earlier one
        rec["point"] = point(rec)
        save()
    if "kernel" in blocks:
        snrs = [float(v) for v in a.snrs.split(",")]
        rec["kernel"] = kernel_alone(a.kernel_frames, 15, snrs[len(snrs) // 2], a.reps)
        save()
    if "speed" in blocks:
        rec["speed"] = {"n64": speed(64, a.n64_frames, 560, a.reps), "cfg4": speed(1024, a.cfg4_frames, 1304, a.reps)}
        save()
    print(json.dumps(rec))

if __name__ == "__main__":
    main()
