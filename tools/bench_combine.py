"""EXT-7 soft combining (ofdm_rx_decode_combine_batch, ofdm_llr_combine_batch; definition: tests/combine_ref.py): what R captures of one
frame deliver next to one, and what combining costs.  Prints one JSON record and writes it to profiles/combine_ber_and_speed.json
(--out).  Runs on tools/link.py's seeded link (branch_link_on): one transmit frame, R channel rows with their own seeds, delays, CFOs.

  sweep    N = 64, 64-QAM, guard bands, LDPC648, payload 560, --frames frames a point, snr_db in 1 dB steps: right (status 0, the true
           length and bytes) / wrong (status 0 otherwise) / reported (any other status) for R = 1, 2, 4 at equal snr_db and for R = 2 with
           branch 1 5 dB down; next to each the combine chain (weighted), every branch alone (ofdm_rx_decode_batch over its rows) and the
           equal-weight sum (the stage with quality = NULL, then the frame rule over k_ldpc_decode's code words).
  point    the snr_db of the skewed sweep at which branch 0 alone delivers nearest to 80 % right: the link
           tests/test_gpu_combine.py::test_combining_earns_its_keep_on_one_link runs.
  speed    65 536 frames of R = 2 captures: the combine chain next to R single decode passes, alternated in one process, --reps passes
           each, with spread.
  kernel   k_llr_combine alone on the speed block's LLR rows (R = 2 and R = 4): bytes moved ((R + 1) rows a frame) per second next to
           ofdm_hbm_read_probe pattern 2 (unit-stride 16-byte loads) over a buffer of the same size, alternated in the same process.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ofdm_amd import api  # noqa: E402
from tools.link import alternated_ms, branch_link_on, delivered, median, open_record  # noqa: E402

N, MOD, PAYLOAD, SEED = 64, api.QAM64, 560, 7100
SKEW_DB = 5.0


def contexts(ecc=api.ECC_LDPC648, **kw):
    """(the mode's context, an ECC_NONE context of the same link: its decode_batch gives the front end's status / offset / f_delta alone)"""
    return (api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=ecc, **kw),
            api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=api.ECC_NONE, **kw))


def sweep_seed(snr):
    return SEED + int(round(10 * snr))


def branch_stages(c, c0, rx, D, frame_len=None):
    """The stages of the combine chain over the branch rows of rx [F, R, span], through the stage entry points: the front end's status,
    offset and f_delta (c0.decode_batch), k_rx_prepare's live symbols, the channel estimate, the quality rows and the LLRs."""
    F, R, span = rx.shape
    rows = rx.view(F * R, span)
    frame_len = span if frame_len is None else frame_len
    fe = c0.decode_batch(rows, max_symbols=D, frame_len=frame_len)
    status = fe["status"]
    off = torch.where(status == 0, fe["offset"], torch.zeros_like(fe["offset"]))
    nsym = torch.where(status == 0, torch.clamp(-(-(frame_len - off) // c.S) - 10, max=D), torch.zeros_like(off)).to(torch.int32)
    hk = c.estimate_channel(rows, off, fe["f_delta"], frame_len=frame_len)
    quality = c.rx_quality(rows, 0, 10, None, off, fe["f_delta"], hk, status, frame_len=frame_len)
    llr = c.rx_llr(rows, D, first_symbol=10, offset=off, f_delta=fe["f_delta"], hk=hk, frame_len=frame_len)
    return {"status": status, "offset": fe["offset"], "f_delta": fe["f_delta"], "metric": fe["metric"], "nsym": nsym, "quality": quality,
            "llr": llr, "n_live": (nsym * (c.data_carriers * c.modulation)).to(torch.int32)}


def ldpc648_frame_rule(c, comb, status, nsym):
    """The LDPC648 frame rule of include/ofdm_hip.h over combined LLR rows [F, n_llr] with the merged status and live symbols, the code
    words decoded by k_ldpc_decode (Context.ldpc_decode) -> {"status", "len", "bytes"} as decode_batch returns them"""
    F = comb.shape[0]
    body = nsym.to(torch.int64) * c.bytes_per_symbol - 16
    nb = torch.clamp(body, min=0) // 80
    ncw = (comb.shape[1] - 128) // 640
    by, it = c.ldpc_decode(comb[:, 128:128 + 640 * ncw].contiguous())                     # [F, 40 ncw], [F, ncw]
    by = by.view(F, -1)
    it = it.view(F, ncw)
    word = by[:, :8].to(torch.int64)
    p = word[:, 0] | (word[:, 1] << 8) | (word[:, 2] << 16) | (word[:, 3] << 24)
    inv = word[:, 4] | (word[:, 5] << 8) | (word[:, 6] << 16) | (word[:, 7] << 24)
    st = status.clone()
    live = (st == 0)
    header_bad = live & ((nb == 0) | (it[:, 0] == 0) | (inv != (p ^ 0xFFFFFFFF)))
    st[header_bad] = api.FRAME_HEADER
    need = torch.minimum((p + 8 + 39) // 40, nb)
    idx = torch.arange(ncw, device=comb.device)[None, :]
    unconverged = ((it == 0) & (idx < need[:, None])).any(dim=1)
    st[(st == 0) & unconverged] = api.FRAME_UNCORRECTABLE
    ln = torch.where(st == 0, torch.minimum(p, 40 * nb - 8), torch.zeros_like(p)).to(torch.int32)
    return {"status": st, "len": ln, "bytes": by[:, 8:]}


def stage_decode(c, c0, rx, D, weighted):
    """The chain as a composition of the stage entry points for LDPC648: weighted = the quality rows' weights, else the equal-weight
    sum (ofdm_llr_combine_batch with quality = NULL)"""
    F, R, _ = rx.shape
    s = branch_stages(c, c0, rx, D)
    q = s["quality"]
    live = s["status"] == 0
    if weighted:
        u = q[:, api.Q_LLR_UNIT]
        live = live & (q[:, api.Q_VALID] == 1) & torch.isfinite(u) & (u > 0)
    comb = c.llr_combine(s["llr"], R, q if weighted else None, s["status"], s["n_live"])
    live = live.view(F, R)
    st = s["status"].view(F, R)
    first_bad = torch.gather(st, 1, (st != 0).to(torch.int32).argmax(dim=1, keepdim=True))[:, 0]
    merged = torch.where(live.any(dim=1), torch.zeros_like(first_bad),
                         torch.where((st != 0).any(dim=1), first_bad, torch.full_like(first_bad, api.FRAME_HEADER)))
    nsym = torch.where(live, s["nsym"].view(F, R), torch.zeros_like(st)).max(dim=1).values
    return ldpc648_frame_rule(c, comb, merged, nsym)


def counts(r, pay):
    right, ok = delivered(r, pay, pay.shape[1])
    return {"right": int(right.sum()), "wrong": int((ok & ~right).sum()), "reported": int((~ok).sum())}


def point_counts(c, c0, snrs, n_frames, seed, payload=PAYLOAD):
    """the counts of one sweep point: branch r at snrs[r]"""
    pay, rx = branch_link_on(c, n_frames, payload, snrs, seed)
    D = c.data_symbols(payload)
    row = {"weighted": counts(c.decode_combine(rx, max_symbols=D), pay), "equal_weight": counts(stage_decode(c, c0, rx, D, False), pay)}
    for r in range(len(snrs)):
        row[f"branch{r}"] = counts(c.decode_batch(rx[:, r].contiguous(), max_symbols=D), pay)
    torch.cuda.synchronize()
    return row


def sweep(snrs, n_frames):
    c, c0 = contexts()
    out = {"n_fft": N, "modulation": "64-QAM", "guard_bands": True, "ecc": "LDPC648", "payload": PAYLOAD, "frames_per_point": n_frames,
           "seed": "SEED + 10 snr_db (+ r for branch r's channel)", "skew_db": SKEW_DB, "points": []}
    for snr in snrs:
        row = {"snr_db": snr}
        for name, branches in (("r1", [snr]), ("r2", [snr] * 2), ("r4", [snr] * 4), ("r2_skewed", [snr, snr - SKEW_DB])):
            row[name] = point_counts(c, c0, branches, n_frames, sweep_seed(snr))
        out["points"].append(row)
        torch.cuda.empty_cache()
    return out


def keep_point(rec):
    """the point of the skewed sweep at which branch 0 alone delivers nearest to 80 % right (the lower snr_db of two equally near)"""
    sw = rec["sweep"]
    best = min(sw["points"], key=lambda p: (abs(p["r2_skewed"]["branch0"]["right"] - 0.8 * sw["frames_per_point"]), p["snr_db"]))
    return {"snr_db": best["snr_db"], "frames": sw["frames_per_point"], **best["r2_skewed"]}


def speed(n_frames, R, reps):
    c, _ = contexts()
    D = c.data_symbols(PAYLOAD)
    x = torch.empty((n_frames, R, c.frame_samples(PAYLOAD) + 160), dtype=torch.complex64, device=c.device)
    pays = []
    for lo in range(0, n_frames, 8192):
        hi = min(lo + 8192, n_frames)
        pay, rx = branch_link_on(c, hi - lo, PAYLOAD, [40.0] * R, 4_100_003 + lo)
        x[lo:hi] = rx
        pays.append(pay)
        del rx
    pay = torch.cat(pays)
    rows = x.view(n_frames * R, -1)
    runs = {"combine_chain": (c, lambda: c.decode_combine(x, max_symbols=D)),
            "single_passes": (c, lambda: c.decode_batch(rows, max_symbols=D))}
    ts = alternated_ms(runs, reps)
    r = c.decode_combine(x, max_symbols=D)
    torch.cuda.synchronize()
    out = {"frames": n_frames, "branches": R, "payload": PAYLOAD, "data_symbols": D, "dispatch": c.last_dispatch(),
           "frames_exact": counts(r, pay)["right"]}
    for name in runs:
        out[name] = {"ms_per_pass": median(ts[name]), "ms_all": ts[name], "spread_ms": max(ts[name]) - min(ts[name])}
    out["combine_over_single_passes"] = out["combine_chain"]["ms_per_pass"] / out["single_passes"]["ms_per_pass"]
    return out


def kernel_alone(n_frames, n_llr, reps):
    c, _ = contexts()
    g = torch.Generator(device=c.device); g.manual_seed(3)
    out = {"frames": n_frames, "n_llr": n_llr, "runs": []}
    for R in (2, 4):
        stride = (n_llr + 15) // 16 * 16
        llr = torch.randint(-127, 128, (n_frames * R, stride), dtype=torch.int8, device=c.device, generator=g)[:, :n_llr]
        q = torch.zeros((n_frames * R, api.QUALITY_FIELDS), dtype=torch.float32, device=c.device)
        q[:, api.Q_VALID] = 1.0
        q[:, api.Q_LLR_UNIT] = torch.rand((n_frames * R,), device=c.device, generator=g) * 0.75 + 0.25   # every branch weighs >= 16: all are read
        dst = torch.empty((n_frames, stride), dtype=torch.int8, device=c.device)[:, :n_llr]
        moved = (R + 1) * n_frames * n_llr
        probe = torch.zeros((moved // 8,), dtype=torch.complex64, device=c.device)
        runs = {"k_llr_combine": (c, lambda: c.llr_combine(llr, R, q, out=dst)), "hbm_read_probe_2": (c, lambda: c.hbm_read_probe(probe, 2))}
        ts = alternated_ms(runs, reps)
        k, p = median(ts["k_llr_combine"]), median(ts["hbm_read_probe_2"])
        out["runs"].append({"branches": R, "bytes_moved": moved, "k_llr_combine_ms": k, "k_llr_combine_ms_all": ts["k_llr_combine"],
                            "k_llr_combine_GBps": moved / k / 1e6, "probe_bytes": probe.numel() * 8, "probe_ms": p,
                            "probe_ms_all": ts["hbm_read_probe_2"], "probe_GBps": probe.numel() * 8 / p / 1e6,
                            "share_of_probe": (moved / k) / (probe.numel() * 8 / p)})
        del llr, dst, probe
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="sweep,point,speed,kernel")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--snrs", default="2,3,4,5,6,7,8,9,10,11,12")
    ap.add_argument("--speed-frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_ber_and_speed.json"))
    a = ap.parse_args()
    blocks = a.blocks.split(",")
    rec = {"tool": "tools/bench_combine.py", "device": torch.cuda.get_device_name(0), "llr_scale": api.SOFT_LLR_SCALE,
           "definition": "parity unpinned by the reference: tests/combine_ref.py is the definition"}
    rec, save = open_record(rec, a.out, keep_earlier=True)
    if "sweep" in blocks:
        rec["sweep"] = sweep([float(v) for v in a.snrs.split(",")], a.frames)
        save()
    if "point" in blocks:
        rec["point"] = keep_point(rec)
        save()
    if "speed" in blocks:
        rec["speed"] = speed(a.speed_frames, 2, a.reps)
        save()
    if "kernel" in blocks:
        c = api.Context(n_fft=N, modulation=MOD, guard_bands=True, ecc=api.ECC_LDPC648)
        rec["kernel"] = kernel_alone(a.speed_frames, c.data_symbols(PAYLOAD) * c.data_carriers * c.modulation, a.reps)
        save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
