"""The cases of tests/test_gpu_ws_poison.py: one table, one line per (entry point, mode, setting) whose answer must not depend on what the
context's workspaces and the host pipe's buffers held before the call ("the workspace ledger").  Imports without a GPU:
tests/test_ws_poison_cpu.py holds the table against the WsRole enum and the entry points of include/ofdm_hip.h.

A Case names
  entry   the C entry points its call goes through (the ones the completeness check counts);
  ctx     the options and tuning keys of the context under test;
  build   build(api, big) -> the inputs, made on a maker context of their own and shared by every context under test (the runner caches
          them), so that a context under test has run nothing before the call.  big: twice the rows and a larger max_symbols -- the call
          that forces every workspace to be freed and allocated again in mid-life;
  call    call(ctx, inputs) -> {name: numpy array}: EVERY output the header defines, compared bit for bit.  Bytes of a row behind its
          out_len are unspecified by the header (include/ofdm_hip.h: "Bytes of a row beyond out_len are unspecified") and belong to the
          row-contract tests: rows_out() blanks them, and only them;
  right   right(api, orc, inputs, out): the premise -- the answer of a new context is right by the bar the entry point's own test file
          uses (payloads delivered, statuses as built, the float stages within their file's tolerance of their reference);
  roles   the WsRole names the call must leave allocated: stat_ws_live is held to exactly this set.

Adding a role or an entry point: give it a case here (or a NO_WORKSPACE line with the reason); tests/test_ws_poison_cpu.py is red until
the union of `roles` covers the enum and every `ofdm_ctx *` entry point of the header is named."""
import os
import re
import sys
from typing import Callable, NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALL = 10 ** 6
TOL = 1e-5                                                 # complex samples, norm-relative (tests/test_gpu_variants.py)
FRAME_OK, FRAME_SHORT, FRAME_NOSYNC, FRAME_HEADER, FRAME_UNCORRECTABLE, FRAME_FCS = 0, -1, -2, -4, -5, -6
NOISE = 0.01                                               # amplitude of what lies in front of a shifted frame and of a noise-only row


class Case(NamedTuple):
    id: str
    entry: tuple
    ctx: dict
    build: Callable
    call: Callable
    right: Callable
    roles: frozenset


# ---------------------------------------------------------------------------------------------------------------- the source's lists
def ws_roles():
    """the WsRole enum of ofdm_amd/csrc/ofdm_ctx.hpp, in order, without the kWsRoles count"""
    src = open(os.path.join(ROOT, "ofdm_amd", "csrc", "ofdm_ctx.hpp")).read()
    body = src[src.index("enum WsRole {"):]
    body = body[body.index("{") + 1: body.index("};")]
    body = re.sub(r"//[^\n]*", "", body)
    names = [w.strip() for w in body.split(",") if w.strip()]
    assert names[-1] == "kWsRoles", names[-1]
    return names[:-1]


def ctx_entry_points():
    """every function of include/ofdm_hip.h whose first parameter is the context"""
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    return sorted(set(re.findall(r"^[A-Za-z_][\w ]*?\b(ofdm_\w+)\(\s*(?:const\s+)?ofdm_ctx\s*\*\s*ctx\b", hdr, flags=re.M)))


def role_mask(names):
    order = ws_roles()
    return sum(1 << order.index(n) for n in names)


def mask_names(mask):
    return sorted(n for i, n in enumerate(ws_roles()) if mask >> i & 1)


# ---------------------------------------------------------------------------------------------------------------- outputs
def _np(v):
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def arrays(ctx, **named):
    """named outputs (device tensors, numpy arrays, numbers) as host arrays, after the context's stream has drained"""
    ctx.synchronize()
    return {k: np.ascontiguousarray(np.atleast_1d(_np(v))) for k, v in named.items() if v is not None}


def rows_out(ctx, res, extra=()):
    """a decode result (decode_batch's dict, or decode_long's of one row): status, len, offset, f_delta, metric and the first out_len
    bytes of every row with status 0; everything behind is blanked (unspecified by the header)"""
    out = arrays(ctx, **{k: res[k] for k in ("status", "len", "offset", "f_delta", "metric") + tuple(extra) if k in res})
    by = np.atleast_2d(_np(res["bytes"])).copy()
    keep = np.where(out["status"] == 0, np.clip(out["len"], 0, by.shape[1]), 0)
    by[np.arange(by.shape[1])[None, :] >= keep[:, None]] = 0
    out["bytes"] = by
    return out


def same(a, b):
    """two output dicts, equal bit for bit -> the first field that differs, or None"""
    if sorted(a) != sorted(b):
        return "fields %s / %s" % (sorted(a), sorted(b))
    for k in sorted(a):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            return k
    return None


def rel_err(a, b):
    a, b = np.asarray(a).astype(np.complex128).ravel(), np.asarray(b).astype(np.complex128).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- the standard batch
KINDS6 = ("whole", "whole", "cut", "short", "noise", "whole")
KINDS3 = ("whole", "cut", "noise")


def _noise(ctx, g, shape):
    import torch

    re_im = torch.randn(tuple(shape) + (2,), dtype=torch.float32, device=ctx.device, generator=g) * NOISE
    return torch.view_as_complex(re_im).contiguous()


def std_batch(api, n=64, mod=4, ecc=0, payload=200, snr=30.0, kw=None, kinds=KINDS6, seed=9100, wide=False, abs_cfo=False, big=False, span=None):
    """The rows of tools/link.py's seeded link rebuilt to every kind (the standard batch of every decode case): whole frames; one shifted right by
    3 S + 5 samples (frames of fewer than 4 data symbols: by (D - 1) S + 5 and the 160 samples the link leaves behind a frame), so that the
    capture's end cuts it to fewer live symbols than max_symbols; one shifted so that fewer than 10 S samples remain behind its trimmed
    start (FRAME_SHORT); one row of noise alone (FRAME_NOSYNC).  big: the kinds twice over and twice max_symbols."""
    import torch
    from tools.link import generator, link_on, wide_link_on

    kw = dict(kw or {})
    maker = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, **kw)
    kinds = tuple(kinds) * (2 if big else 1)
    n_link = sum(k != "noise" for k in kinds)
    if wide:
        pay, rx, _, _ = wide_link_on(maker, n_link, payload, snr, seed)
    elif abs_cfo:                                          # the reference's detector reports |f_delta|: a link whose offsets are not negative
        g = generator(maker, seed)
        pay = torch.randint(0, 256, (n_link, payload), dtype=torch.uint8, device=maker.device, generator=g)
        tx = maker.encode_batch(pay)
        d = torch.randint(1, 33, (n_link,), dtype=torch.int32, device=maker.device, generator=g)
        fd = torch.rand((n_link,), dtype=torch.float64, device=maker.device, generator=g) / maker.S
        rx = maker.channel_batch(tx, snr_db=snr, seed=seed, delay=d, f_delta=fd, span=tx.shape[1] + 160)
    else:
        pay, rx = link_on(maker, n_link, payload, snr, seed)
    assert span in (None, rx.shape[1]), (span, rx.shape[1])   # what the case's search roles were worked out for (sc64)
    S, span, D = maker.S, rx.shape[1], maker.data_symbols(payload)
    g = generator(maker, seed + 1)
    rows = _noise(maker, g, (len(kinds), span))
    sent = torch.zeros((len(kinds), payload), dtype=torch.uint8, device=maker.device)
    cut = 3 * S + 5 if D >= 4 else (D - 1) * S + 5 + 160
    short = span - 8 * S
    assert 0 < cut < span and short > 0
    k = 0
    for f, kind in enumerate(kinds):
        if kind == "noise":
            continue
        s = {"whole": 0, "cut": cut, "short": short}[kind]
        rows[f, s:] = rx[k, : span - s]
        sent[f] = pay[k]
        k += 1
    maker.synchronize()
    return {"rx": rows.contiguous(), "pay": sent.cpu().numpy(), "kinds": kinds, "D": D * (2 if big else 1), "payload": payload,
            "S": S, "n": n, "mod": mod, "ecc": ecc, "kw": kw, "span": span, "bps": maker.bytes_per_symbol}


def cut_status(ecc):
    """What a mode makes of the standard batch's cut row (include/ofdm_hip.h): without an outer layer every inner mode delivers the prefix
    it still holds (status 0).  An RS mode decodes the shortened row as a zero-padded block: the 120-byte payload's one block loses the
    end of its 32 parity bytes only (the frame's last symbol holds 7 bytes of the block, the tail chunk before it 12), which 16
    corrections reach -- status 0 and, checked by decode_right, the payload itself, so also behind the frame check.  A frame check over a
    prefix that no outer code repairs is FRAME_FCS"""
    fcs = ecc >= A.ECC_FCS
    base = ecc - A.ECC_FCS if fcs else ecc
    if A.ECC_RS255 <= base <= A.ECC_RS255_K7F_R34:
        return FRAME_OK
    return FRAME_FCS if fcs else FRAME_OK


def decode_right(statuses=True):
    """whole rows deliver the payload that was sent (an RS mode without the frame check delivers its padding too: tools/link.py,
    delivered(exact=False)); the built rows have the statuses they were built for.  A row cut by its capture's end delivers, without a
    code, fewer bytes than were sent -- those of its whole symbols are the payload's, the last live symbol is the reference's zero-padded
    tail chunk (receiver.rs, split_into_chunks) -- and with a code the one status cut_status() names for the mode.  statuses=False (the reference's detector, an argmax that always finds something): the whole rows
    only."""
    def right(api, orc, inp, out):
        p = inp["payload"]
        padded = A.ECC_RS255 <= inp["ecc"] <= A.ECC_RS255_K7F_R34
        for f, kind in enumerate(inp["kinds"]):
            st, ln = int(out["status"][f]), int(out["len"][f])
            what = (f, kind, st, ln)
            if kind == "whole":
                assert st == FRAME_OK and (ln >= p if padded else ln == p) and bytes(out["bytes"][f, :p]) == bytes(inp["pay"][f]), what
            elif not statuses:
                continue
            elif kind == "short":
                assert st == FRAME_SHORT and ln == 0, what
            elif kind == "noise":
                assert st == FRAME_NOSYNC and ln == 0, what
            else:
                assert st == cut_status(inp["ecc"]), what + (cut_status(inp["ecc"]),)
                if st != FRAME_OK:
                    assert ln == 0, what
                elif ln >= p:                             # an outer code repaired the cut: the payload, not just a status
                    assert bytes(out["bytes"][f, :p]) == bytes(inp["pay"][f]), what
                elif inp["ecc"] == 0:
                    whole = (inp["span"] - int(out["offset"][f]) - 10 * inp["S"]) // inp["S"]
                    n_cmp = min(ln, whole * inp["bps"] - 16)
                    assert 0 <= ln < p and (n_cmp <= 0 or bytes(out["bytes"][f, :n_cmp]) == bytes(inp["pay"][f, :n_cmp])), what + (n_cmp,)
    return right


def decode_call(ctx, inp):
    return rows_out(ctx, ctx.decode_batch(inp["rx"], inp["D"]))


def decode_odd_stride_call(ctx, inp):
    """ofdm_rx_decode_batch into rows an odd number of bytes apart: the fused kernel leaves the finish to k_rx_finish"""
    import torch

    import rows as R

    n = inp["rx"].shape[0]
    ob = ctx.decode_row_bytes(inp["D"]) | 1
    out = torch.empty((n, ob), dtype=torch.uint8, device=ctx.device)
    res = {"bytes": out, "len": ctx.empty((n,), torch.int32), "status": ctx.empty((n,), torch.int32), "offset": ctx.empty((n,), torch.int32),
           "f_delta": ctx.empty((n,), torch.float64), "metric": ctx.empty((n,), torch.float32)}
    rc = R.rx_decode(ctx, inp["rx"], n, inp["rx"].shape[1], inp["rx"].shape[1], 0, inp["D"], out, ob, res["len"], res["status"], res["offset"],
                     res["f_delta"], res["metric"])
    assert rc == 0, rc
    return rows_out(ctx, res)


def decode_host_call(ctx, inp):
    return rows_out(ctx, ctx.decode_host(inp["rx_np"], inp["D"], chunk_frames=4))


def with_host(build):
    """the builder's device rows also as a host array"""
    def b(api, big):
        inp = build(api, big)
        inp["rx_np"] = inp["rx"].cpu().numpy()
        return inp
    return b


def with_sc16(build, key="rx"):
    """the builder's rows quantised with their peak at 0.9 of full scale (tests/sc16_ref.py), on the device and on the host"""
    def b(api, big):
        import torch

        import sc16_ref

        inp = build(api, big)
        q, scale = sc16_ref.quantise(inp[key].cpu().numpy(), 0.9)
        inp["q_np"], inp["scale"] = np.ascontiguousarray(q), float(scale)
        inp["q"] = torch.from_numpy(inp["q_np"]).to(inp[key].device)
        return inp
    return b


# roles by what the chain takes (ofdm_abi.hip: rx_front_end, rx_decode_inner, rx_finish_soft, rx_decode_run)
FRONT = frozenset({"kWsDhat", "kWsFdelta", "kWsOffset", "kWsNsym", "kWsRaw"})
FUSED64 = FRONT | {"kWsCut"}
SOFT64 = FRONT | {"kWsHk", "kWsLlr"}
VIT64 = SOFT64 | {"kWsSurvivors"}


def sc64(span):
    """What the N = 64 search of a small batch of even rows of `span` samples takes (sc_run_impl, ofdm_abi.hip): rows of up to 2560 samples
    go through the filter kernels, whose candidate lists live in kWsSearch (sc_fast_ok / sc80_wanted: n_lags + W + L <= 2560); longer
    rows of up to 2560 lags are one tile of k_sc_tile, which takes nothing; beyond that the tiled search keeps its crossings per tile in
    kWsSearch and the first one per row in kWsSearchD1.  (N >= 128: k_sc_stream, which takes nothing.)"""
    assert span % 2 == 0
    if span <= 2560:
        return frozenset({"kWsSearch"})
    return frozenset() if span - 4 * 80 + 1 <= 2560 else frozenset({"kWsSearch", "kWsSearchD1"})


def span64(coded_bytes, mod):
    """samples of a row of the seeded link at N = 64 with guard bands: the ten header blocks, the data symbols of 16 + coded_bytes bytes, and the
    160 samples the link leaves behind the frame"""
    return (10 + -(-(16 + coded_bytes) * 8 // (48 * mod))) * 80 + 160


def _decode_specs(api_consts):
    A = api_consts
    coded = dict(mod=2, payload=120, snr=25.0)
    plain = dict(mod=4, payload=200, snr=30.0, span=span64(200, 4))
    # the coded bytes of 120 payload bytes, by the length maps of ofdm_ctx.hpp (inner_coded_bytes, outer_coded_bytes)
    ham = span64(30 * 7, 2)                                # ((n + 3) / 4) * 7
    k7 = span64(2 * 121, 2)                                # 2 (n + 1)
    k7f_r34 = span64(18 + 162, 2)                          # the length block, then ceil(8 * 121 * 4 / 3 / 8) bytes
    ldpc = span64(4 * 80, 2)                               # 8 + 120 info bytes in code words of 40
    fcs_ldpc_r34 = span64(3 * 80, 2)                       # 8 + 128 info bytes in code words of 60
    rs = span64(255, 2)                                    # one RS(255,223) block (the frame check's 8 bytes fit it too)
    rs_k7f_r12 = span64(18 + 2 * 256, 2)
    # id -> (std_batch options, tuning, roles)
    specs = {
        "none": (dict(plain, ecc=A.ECC_NONE), {}, FUSED64 | sc64(plain["span"])),
        "hamming74": (dict(coded, ecc=A.ECC_HAMMING74, span=ham), {}, FUSED64 | sc64(ham)),
        "hamming74_soft": (dict(coded, ecc=A.ECC_HAMMING74_SOFT, span=ham), {}, SOFT64 | sc64(ham)),
        "conv_k7": (dict(coded, ecc=A.ECC_CONV_K7, span=k7), {}, VIT64 | sc64(k7)),
        "conv_k7f_r34": (dict(coded, ecc=A.ECC_CONV_K7F_R34, span=k7f_r34), {}, VIT64 | sc64(k7f_r34)),
        "ldpc648": (dict(coded, ecc=A.ECC_LDPC648, span=ldpc), {}, SOFT64 | sc64(ldpc)),
        "fcs_ldpc648_r34": (dict(coded, ecc=A.ECC_FCS + A.ECC_LDPC648_R34, span=fcs_ldpc_r34), {}, SOFT64 | sc64(fcs_ldpc_r34) | {"kWsRxFcsRows"}),
        "rs255": (dict(coded, ecc=A.ECC_RS255, span=rs), {}, FUSED64 | sc64(rs) | {"kWsRxRsRows"}),
        "rs255_k7f_r12": (dict(coded, ecc=A.ECC_RS255_K7F_R12, span=rs_k7f_r12), {}, VIT64 | sc64(rs_k7f_r12) | {"kWsRxRsRows"}),
        "fcs_rs255": (dict(coded, ecc=A.ECC_FCS + A.ECC_RS255, span=rs), {}, FUSED64 | sc64(rs) | {"kWsRxFcsRows", "kWsRxRsRows"}),
        "chest_wls": (dict(plain, ecc=A.ECC_NONE, kw=dict(chest_mode=A.CHEST_WLS)), {}, FRONT | sc64(plain["span"]) | {"kWsHk", "kWsChestTaps"}),
        "cfo_wide": (dict(coded, ecc=A.ECC_CONV_K7F_R34, kw=dict(cfo_mode=A.CFO_WIDE), wide=True, span=k7f_r34), {}, VIT64 | sc64(k7f_r34)),
        "llrw_noise_ldpc648": (dict(coded, ecc=A.ECC_LDPC648, kw=dict(llr_weight=A.LLRW_NOISE), span=ldpc), {}, SOFT64 | sc64(ldpc) | {"kWsNoiseWeight"}),
        # the reference's detector: k_xcorr's tile maxima live in kWsSearch whatever the row length
        "sync_reference": (dict(plain, ecc=A.ECC_NONE, kw=dict(sync_mode=A.SYNC_REFERENCE), abs_cfo=True), {}, FUSED64 | {"kWsSearch"}),
        # the generic chain and kWsHk; the fused N = 1024 frame kernel; the largest N with max_symbols 2 (30 dB at the data symbols: data_snr)
        "n256_none": (dict(plain, n=256, ecc=A.ECC_NONE, snr=30.0 + 10 * np.log10(4), span=None), {}, FRONT | {"kWsHk"}),
        "n1024_hamming74": (dict(coded, n=1024, ecc=A.ECC_HAMMING74, snr=30.0 + 10 * np.log10(16), kinds=KINDS3), {}, FRONT),
        "n4096_none": (dict(mod=2, payload=1200, n=4096, ecc=A.ECC_NONE, snr=30.0 + 10 * np.log10(64), kinds=KINDS3), {}, FRONT | {"kWsHk"}),
    }
    soft = ("hamming74_soft", "conv_k7", "conv_k7f_r34", "ldpc648", "fcs_ldpc648_r34", "rs255_k7f_r12", "cfo_wide", "llrw_noise_ldpc648")
    for s in soft:                                         # a chunk of 4 rows, then a chunk of 2 over the LLR rows the first one left
        opt, tune, roles = specs[s]
        specs[s + "-chunk4"] = (opt, {**tune, "soft_chunk_frames": 4}, roles)
    return specs


class _ApiConsts:
    """the constants of ofdm_amd/api.py the table needs, restated so that this module imports without torch (test_ws_poison_cpu.py
    holds them to api.py's when that imports)"""
    ECC_NONE, ECC_HAMMING74, ECC_HAMMING74_SOFT, ECC_CONV_K7 = 0, 1, 2, 5
    ECC_CONV_K7F_R12, ECC_CONV_K7F_R34 = 10, 12
    ECC_RS255, ECC_RS255_K7F_R12, ECC_RS255_K7F_R34 = 20, 30, 32
    ECC_FCS, ECC_LDPC648, ECC_LDPC648_R34 = 64, 16, 42
    CFO_WIDE, SYNC_REFERENCE, CHEST_WLS, LLRW_NOISE = 3, 1, 1, 1
    CONV_RATE_3_4 = 2


A = _ApiConsts


def _ctx_of(opt, tuning):
    """api.Context options of a std_batch spec"""
    return dict(n_fft=opt.get("n", 64), modulation=opt["mod"], guard_bands=True, ecc=opt["ecc"], tuning=dict(tuning), **opt.get("kw", {}))


def _std_builder(opt):
    return lambda api, big: std_batch(api, big=big, **opt)


def decode_cases():
    out = []
    for name, (opt, tuning, roles) in _decode_specs(A).items():
        right = decode_right(statuses=name != "sync_reference")
        out.append(Case("decode_batch-" + name, ("ofdm_rx_decode_batch",), _ctx_of(opt, tuning), _std_builder(opt), decode_call, right, frozenset(roles)))
    opt, tuning, roles = _decode_specs(A)["none"]
    out.append(Case("decode_batch-none-odd_out_stride", ("ofdm_rx_decode_batch",), _ctx_of(opt, tuning), _std_builder(opt), decode_odd_stride_call,
                    decode_right(), frozenset(roles)))
    # the host form in chunks of 4 of 6: three slots, a short last chunk, pageable memory through the pinned bounce slots
    out.append(Case("decode_host-none-chunk4", ("ofdm_rx_decode_host",), _ctx_of(opt, tuning), with_host(_std_builder(opt)), decode_host_call,
                    decode_right(), frozenset(roles)))
    return out


# ---------------------------------------------------------------------------------------------------------------- sc16 receive
def decode_sc16_call(ctx, inp):
    return rows_out(ctx, ctx.decode_batch_sc16(inp["q"], inp["D"], scale=inp["scale"]))


def decode_host_sc16_call(ctx, inp):
    return rows_out(ctx, ctx.decode_host_sc16(inp["q_np"], inp["D"], chunk_frames=4, scale=inp["scale"]))


def stream_batch(api, big, n_frames=6, syms=18):
    """regular QPSK symbol streams (the data symbols of the context's own frames: QPSK decisions do not depend on the frame's scale)"""
    import torch
    from tools.link import generator

    maker = api.Context(n_fft=64, modulation=2, guard_bands=True)
    nf = n_frames * (2 if big else 1)
    payload = syms * maker.bytes_per_symbol - 16
    g = generator(maker, 9300)
    pay = torch.randint(0, 256, (nf, payload), dtype=torch.uint8, device=maker.device, generator=g)
    tx = maker.encode_batch(pay)
    assert maker.data_symbols(payload) == syms
    x = tx[:, 10 * maker.S:].contiguous()
    maker.synchronize()
    return {"x": x, "x_np": x.cpu().numpy(), "pay": pay.cpu().numpy(), "syms": syms, "payload": payload}


def stream_right(api, orc, inp, out):
    by = out["bytes"]
    assert by.shape[1] == 16 + inp["payload"]
    assert np.array_equal(by[:, 16:], inp["pay"]) and np.array_equal(np.ascontiguousarray(by[:, :8]).view(np.uint64).ravel(), np.full(by.shape[0], inp["payload"], np.uint64))


def sc16_cases():
    opt, _, roles = _decode_specs(A)["none"]
    chunked = {"sc16_chunk_frames": 4}
    b = with_sc16(_std_builder(opt))
    return [
        Case("decode_batch_sc16-none-chunk4", ("ofdm_rx_decode_sc16_batch",), _ctx_of(opt, chunked), b, decode_sc16_call, decode_right(),
             frozenset(roles | {"kWsSc16"})),
        Case("decode_host_sc16-none-chunk4", ("ofdm_rx_decode_sc16_host",), _ctx_of(opt, chunked), b, decode_host_sc16_call, decode_right(),
             frozenset(roles | {"kWsSc16"})),
        Case("rx_demod_sc16-widen-chunk4", ("ofdm_rx_demod_sc16_batch",),
             dict(n_fft=64, modulation=2, guard_bands=True, tuning={"no_demod64_sc16": 1, "sc16_chunk_frames": 4}), with_sc16(stream_batch, "x"),
             lambda ctx, inp: arrays(ctx, bytes=ctx.rx_demod_sc16(inp["q"], inp["syms"], scale=inp["scale"])), stream_right, frozenset({"kWsSc16"})),
        Case("demod_host_sc16-widen-chunk4", ("ofdm_rx_demod_sc16_host",),
             dict(n_fft=64, modulation=2, guard_bands=True, tuning={"no_demod64_sc16": 1, "sc16_chunk_frames": 3}), with_sc16(stream_batch, "x"),
             lambda ctx, inp: arrays(ctx, bytes=ctx.demod_host_sc16(inp["q_np"], inp["syms"], chunk_frames=4, scale=inp["scale"])), stream_right,
             frozenset({"kWsSc16"})),
        Case("demod_host-chunk4", ("ofdm_rx_demod_host",), dict(n_fft=64, modulation=2, guard_bands=True), stream_batch,
             lambda ctx, inp: arrays(ctx, bytes=ctx.demod_host(inp["x_np"], inp["syms"], chunk_frames=4)), stream_right, frozenset()),
    ]


# ---------------------------------------------------------------------------------------------------------------- search
def search_batch(n, mod, payload, min_span=0, late=(), tile=1):
    """five frames of the seeded link (ten: big) and a row of noise alone, rows of at least min_span samples.  late: frames 2 and 3 start
    that many samples into their rows (their peak windows reach beyond the filter pair's first launch: the redo list).  tile: the rows
    repeated so many times over (k_sc80 takes long rows from 512 rows on)"""
    def build(api, big):
        import torch
        from tools.link import generator, link_on

        maker = api.Context(n_fft=n, modulation=mod, guard_bands=True)
        nf = 10 if big else 5
        pay, rx = link_on(maker, nf, payload, 30.0 + 10 * np.log10(n / 64), 9400 + n)
        span = max(rx.shape[1], min_span + (48 if big else 0))
        g = generator(maker, 9401)
        rows = _noise(maker, g, (nf + 1, span))            # the last row: noise alone
        for f in range(nf):
            s = late[f % 5 - 2] if late and f % 5 in (2, 3) else 0
            rows[f, s: s + rx.shape[1]] = rx[f]
        maker.synchronize()
        uniq = rows.cpu().numpy()
        reps = tile * (2 if big and tile > 1 else 1)
        if reps > 1:
            rows = rows.repeat(reps, 1)
        return {"rx": rows.contiguous(), "rx_np": uniq, "S": maker.S, "n_lags": 0}
    return build


def search_call(ctx, inp):
    d, fd, m = ctx.sc_correlate(inp["rx"], n_lags=inp["n_lags"])
    return arrays(ctx, d_hat=d, f_delta=fd, metric=m)


def search_right(api, orc, inp, out):
    """the f64 oracle's lag exactly, its CFO within 1e-9 and its metric within 1e-6 max(1, metric) (tests/test_gpu_variants.py)"""
    u = len(inp["rx_np"])                                  # (a tiled batch repeats these rows: the oracle runs once per distinct row)
    want = [orc.sc_sync(row.astype(np.complex128), L=inp["S"], window_reps=3, n_lags=inp["n_lags"], threshold=0.5) for row in inp["rx_np"]]
    assert out["d_hat"].size % u == 0
    for f in range(out["d_hat"].size):
        wd, _, wm, wfd = want[f % u]
        assert int(out["d_hat"][f]) == wd, (f, int(out["d_hat"][f]), wd)
        if wd >= 0:
            assert abs(out["f_delta"][f] - wfd) <= 1e-9 and abs(out["metric"][f] - wm) <= 1e-6 * max(1.0, wm), f
    assert all(w[0] >= 0 for w in want[:-1]) and want[-1][0] == -1


def search_cases():
    c64 = dict(n_fft=64, modulation=4, guard_bands=True)
    c128 = dict(n_fft=128, modulation=4, guard_bands=True)
    b64, b128 = search_batch(64, 4, 200), search_batch(128, 4, 300)
    b64_late = search_batch(64, 4, 200, min_span=2176, late=(300, 420))
    b64_long = search_batch(64, 4, 200, min_span=6000, late=(3011, 37), tile=86)      # 6 x 86 = 516 rows of 6000 samples
    b128_tiles = search_batch(128, 4, 300, min_span=2560 + 5 * 160 + 2)     # more lags than one tile of k_sc_tile holds
    e = ("ofdm_sc_correlate_batch",)
    S = frozenset({"kWsSearch"})
    assert sc64(span64(200, 4)) == S
    return [
        Case("sc_correlate-n64", e, c64, b64, search_call, search_right, S),
        Case("sc_correlate-n64-no_sc80", e, dict(c64, tuning={"no_sc80": 1}), b64, search_call, search_right, S),
        # the rows of tests/test_gpu_variants.py that feed the same lists through another instantiation, schedule or list split: k_sc80<1>;
        # the filter pair on rows of 2176 samples with two late packets (the redo list), two wavefronts a frame in the 128-chunk kernel,
        # one launch instead of two, one workgroup a CU; k_sc80 on 516 long rows (the slow list, crossings per tile, the peak launch)
        Case("sc_correlate-n64-sc80_depth1", e, dict(c64, tuning={"sc80_depth": 1}), b64_late, search_call, search_right, S),
        Case("sc_correlate-n64-no_sc80-late", e, dict(c64, tuning={"no_sc80": 1}), b64_late, search_call, search_right, S),
        Case("sc_correlate-n64-no_sc80-two_waves", e, dict(c64, tuning={"no_sc80": 1, "sc128_one_wave": 0}), b64_late, search_call, search_right, S),
        Case("sc_correlate-n64-no_sc80-one_launch", e, dict(c64, tuning={"no_sc80": 1, "sc_first_lags": 0}), b64_late, search_call, search_right, S),
        Case("sc_correlate-n64-no_sc80-one_wg_per_cu", e, dict(c64, tuning={"no_sc80": 1, "sc_wg_per_cu": 1}), b64_late, search_call, search_right, S),
        Case("sc_correlate-n64-sc80-long_rows", e, dict(c64, tuning={"grid_cap": 1}), b64_long, search_call, search_right, S),
        Case("sc_correlate-n64-sc80_depth1-long_rows", e, dict(c64, tuning={"grid_cap": 1, "sc80_depth": 1}), b64_long, search_call, search_right, S),
        Case("sc_correlate-n128-no_sc_stream", e, dict(c128, tuning={"no_sc_stream": 1}), b128_tiles, search_call, search_right, S),
        Case("sc_correlate-n128-two_segments", e, dict(c128, tuning={"no_sc_stream": 1, "scb_two_segments": 1}), b128_tiles, search_call, search_right, S),
        Case("sc_correlate-n128-tiles", e, dict(c128, tuning={"no_sc_stream": 1, "no_sc_big": 1}), b128_tiles, search_call, search_right,
             S | {"kWsSearchD1"}),
    ]


# ---------------------------------------------------------------------------------------------------------------- combine
def combine_batch(ecc):
    def build(api, big):
        from tools.link import branch_link_on, generator

        maker = api.Context(n_fft=64, modulation=2, guard_bands=True, ecc=ecc)
        nf = 6 if big else 3
        pay, rx = branch_link_on(maker, nf, 120, (25.0, 22.0), 9500 + ecc)
        rx = rx.clone()
        rx[1, 1] = _noise(maker, generator(maker, 9501), (rx.shape[2],))       # one branch row of noise alone
        maker.synchronize()
        return {"rx": rx.contiguous(), "pay": pay.cpu().numpy(), "D": maker.data_symbols(120) * (2 if big else 1), "payload": 120, "ecc": ecc}
    return build


def combine_call(ctx, inp):
    r = ctx.decode_combine(inp["rx"], inp["D"])
    out = rows_out(ctx, {k: r[k] for k in ("bytes", "len", "status")} | {k: r[k].reshape(-1) for k in ("offset", "f_delta", "metric")})
    out.update(arrays(ctx, branch_status=r["branch_status"], weight=r["weight"], quality=r["quality"]))
    return out


def combine_bare_call(ctx, inp):
    """ofdm_rx_decode_combine_batch without its optional per-branch outputs: the branch statuses and quality rows live in the workspace"""
    import torch

    import rows as R

    n, Rb, stride = inp["rx"].shape
    ob = ctx.decode_row_bytes(inp["D"])
    res = {"bytes": ctx.empty((n, ob), torch.uint8), "len": ctx.empty((n,), torch.int32), "status": ctx.empty((n,), torch.int32)}
    p = R._p
    rc = ctx.lib.ofdm_rx_decode_combine_batch(ctx.h, p(inp["rx"]), n, Rb, stride, stride, 0, inp["D"], p(res["bytes"]), ob, p(res["len"]), p(res["status"]),
                                             None, None, None, None, None, None)
    assert rc == 0, rc
    ctx.synchronize()
    by = res["bytes"].cpu().numpy().copy()
    st, ln = res["status"].cpu().numpy(), res["len"].cpu().numpy()
    keep = np.where(st == 0, np.clip(ln, 0, ob), 0)
    by[np.arange(ob)[None, :] >= keep[:, None]] = 0
    return {"status": st, "len": ln, "bytes": by}


def combine_reference(api, orc, inp, out):
    """tests/test_gpu_combine.py's bar: the per-branch outputs are the stage entry points' (tools/bench_combine.py, branch_stages) bit for
    bit and the weights are tests/combine_ref.py's; tests/test_gpu_quality.py's bar: the quality rows against tests/quality_ref.py"""
    import combine_ref as cb
    from test_gpu_quality import _assert_rows, _reference
    from tools.bench_combine import branch_stages

    rx = inp["rx"]
    F, R, span = rx.shape
    c = api.Context(n_fft=64, modulation=2, guard_bands=True, ecc=inp["ecc"])
    c0 = api.Context(n_fft=64, modulation=2, guard_bands=True)
    s = {k: v.cpu().numpy() for k, v in branch_stages(c, c0, rx, inp["D"]).items()}
    for k, sk in (("branch_status", "status"), ("offset", "offset"), ("f_delta", "f_delta"), ("metric", "metric"), ("quality", "quality")):
        assert out[k].reshape(-1).tobytes() == s[sk].reshape(-1).tobytes(), k
    with np.errstate(all="ignore"):
        _, q = cb.combine(s["llr"], R, s["quality"], s["status"], s["n_live"])
    assert np.array_equal(out["weight"].reshape(-1), q)
    rows = rx.view(F * R, span)
    off = np.where(s["status"] == 0, s["offset"], 0).astype(np.int32)
    hk = c.estimate_channel(rows, c.to_device(off), c.to_device(s["f_delta"])).cpu().numpy()
    want, tol, near, widen, _ = _reference(rows.cpu().numpy(), 64, True, 2, orc.default_training(64), 0, None, offset=off, f_delta=s["f_delta"], hk=hk,
                                           status=s["status"])
    _assert_rows(out["quality"].reshape(F * R, -1), want, tol, near, widen, "combine")
    c.close(); c0.close()


def combine_right(api, orc, inp, out):
    if "quality" in out:
        combine_reference(api, orc, inp, out)
    p = inp["payload"]
    for f in range(out["status"].size):
        assert int(out["status"][f]) == 0 and int(out["len"][f]) == p and bytes(out["bytes"][f, :p]) == bytes(inp["pay"][f]), f
    if "branch_status" in out:
        bst = out["branch_status"].reshape(-1)
        assert bst[3] == FRAME_NOSYNC and (np.delete(bst, 3)[: 5] == 0).all(), bst
        assert out["weight"].reshape(-1)[3] == 0


def combine_cases():
    e = ("ofdm_rx_decode_combine_batch",)
    base = frozenset({"kWsDhat", "kWsFdelta", "kWsOffset", "kWsNsym", "kWsHk", "kWsLlr", "kWsCombinedNsym"})
    k7f_r12, fcs_ldpc = span64(18 + 2 * 121, 2), span64(4 * 80, 2)      # (8 + 128 info bytes in code words of 40)
    out = []
    for name, ecc, roles in (("k7f_r12", A.ECC_CONV_K7F_R12, base | sc64(k7f_r12) | {"kWsSurvivors"}),
                             ("fcs_ldpc648", A.ECC_FCS + A.ECC_LDPC648, base | sc64(fcs_ldpc) | {"kWsRxFcsRows"})):
        ctx = dict(n_fft=64, modulation=2, guard_bands=True, ecc=ecc, tuning={"soft_chunk_frames": 2})
        out.append(Case("decode_combine-" + name, e, ctx, combine_batch(ecc), combine_call, combine_right, frozenset(roles)))
        out.append(Case("decode_combine-" + name + "-bare", e, ctx, combine_batch(ecc), combine_bare_call, combine_right,
                        frozenset(roles | {"kWsBranchStatus", "kWsBranchQuality"})))
    return out


# ---------------------------------------------------------------------------------------------------------------- transmit
def payload_batch(n_frames, payload, ragged, seed, ecc=0, mod=4):
    def build(api, big):
        rng = np.random.default_rng(seed)
        nf = n_frames * (2 if big else 1)
        nb = payload + (40 if big else 0)
        pay = rng.integers(0, 256, (nf, nb), dtype=np.uint8)
        lens = None
        if ragged:
            lens = rng.integers(1, nb, nf).astype(np.int32)
            lens[0], lens[-1] = nb, 0
        return {"pay_np": pay, "lens_np": lens, "payload": nb, "ecc": ecc, "mod": mod}
    return build


def _dev_payload(ctx, inp):
    import torch

    pay = ctx.to_device(inp["pay_np"])
    lens = None if inp["lens_np"] is None else torch.from_numpy(inp["lens_np"]).to(ctx.device)
    return pay, lens


def encode_call(ctx, inp):
    pay, lens = _dev_payload(ctx, inp)
    return arrays(ctx, frames=ctx.encode_batch(pay, lens=lens))


def encode_host_call(ctx, inp):
    return arrays(ctx, frames=ctx.encode_host(inp["pay_np"], lens=inp["lens_np"], chunk_frames=4))


def encode_right(api, orc, inp, out):
    """no code: the f64 oracle's frame within TOL; coded: a new receiver of the same mode delivers every row's own length and bytes from
    the frames as they stand (40 zeros in front, 160 behind)"""
    frames = out["frames"]
    lens = inp["lens_np"] if inp["lens_np"] is not None else np.full(frames.shape[0], inp["payload"], np.int32)
    if inp["ecc"] == 0:
        for f in range(frames.shape[0]):
            want = orc.encode(bytes(inp["pay_np"][f, : lens[f]]), True, inp["mod"], 64)
            assert rel_err(frames[f, : want.size], want) <= TOL, (f, rel_err(frames[f, : want.size], want))
            assert abs(max(frames[f].real.max(), frames[f].imag.max()) - 1.0) < 1e-6, f
        return
    rx = api.Context(n_fft=64, modulation=inp["mod"], guard_bands=True, ecc=inp["ecc"])
    cap = np.zeros((frames.shape[0], frames.shape[1] + 200), np.complex64)
    cap[:, 40: 40 + frames.shape[1]] = frames
    got = rows_out(rx, rx.decode_batch(rx.to_device(cap), rx.data_symbols(inp["payload"])))
    for f in range(frames.shape[0]):
        assert int(got["status"][f]) == 0 and int(got["len"][f]) == lens[f], (f, int(got["status"][f]), int(got["len"][f]), int(lens[f]))
        assert bytes(got["bytes"][f, : lens[f]]) == bytes(inp["pay_np"][f, : lens[f]]), f


def normalize_build(api, big):
    rng = np.random.default_rng(9600)
    nf, ln = (12, 1531) if big else (6, 1043)              # odd lengths: frame_stride == frame_len, rows on 8-byte boundaries only
    x = ((rng.standard_normal((nf, ln)) + 1j * rng.standard_normal((nf, ln))) * rng.uniform(0.1, 40.0, (nf, 1))).astype(np.complex64)
    return {"x_np": x}


def normalize_call(ctx, inp):
    return arrays(ctx, frames=ctx.normalize(ctx.to_device(inp["x_np"]).clone()))


def normalize_right(api, orc, inp, out):
    """src/transmitter.rs:183-194 as the f64 oracle runs it"""
    for f, row in enumerate(inp["x_np"]):
        want = orc.normalize(row.astype(np.complex128))
        assert rel_err(out["frames"][f], want) <= TOL, (f, rel_err(out["frames"][f], want))


def encode_sc16_call(scale):
    def call(ctx, inp):
        pay, lens = _dev_payload(ctx, inp)
        q, clipped = ctx.encode_batch_sc16(pay, scale, lens=lens, want_clipped=True)
        return arrays(ctx, frames=q, clipped=clipped)
    return call


def encode_host_sc16_call(scale):
    def call(ctx, inp):
        q, clipped = ctx.encode_host_sc16(inp["pay_np"], scale, lens=inp["lens_np"], chunk_frames=4, want_clipped=True)
        return arrays(ctx, frames=q, clipped=clipped)
    return call


def encode_sc16_right(scale):
    def right(api, orc, inp, out):
        """row f = sc16_narrow(frame f of encode_batch, scale), exactly (tests/sc16_ref.py), the fc32 frames being the oracle's within TOL"""
        import sc16_ref

        ref = api.Context(n_fft=64, modulation=inp["mod"], guard_bands=True, ecc=inp["ecc"])
        fc = encode_call(ref, inp)["frames"]
        encode_right(api, orc, inp, {"frames": fc})
        q, _ = sc16_ref.narrow(fc, scale)
        assert np.array_equal(out["frames"], q)
        want_clip = np.array([sc16_ref.narrow(r, scale)[1] for r in fc], np.int32)
        assert np.array_equal(out["clipped"], want_clip)
    return right


def transmit_cases():
    coded = A.ECC_FCS + A.ECC_RS255_K7F_R34
    tx_roles = frozenset({"kWsTxFcsRows", "kWsTxFcsLen", "kWsTxRsRows", "kWsTxRsLen", "kWsTxCoded", "kWsTxCodedLen"})
    plain = dict(n_fft=64, modulation=4, guard_bands=True)
    sc = 30000.0
    return [
        # the generic pair k_sym<tx> + k_tx_finish: the per-frame maxima go through kWsFrameMax
        Case("encode_batch-none-generic", ("ofdm_tx_encode_batch",), dict(plain, tuning={"no_txframe64": 1, "no_mid_kernels": 1}),
             payload_batch(6, 200, True, 9601), encode_call, encode_right, frozenset({"kWsFrameMax"})),
        Case("encode_batch-fcs_rs255_k7f_r34-ragged", ("ofdm_tx_encode_batch",), dict(plain, modulation=2, ecc=coded),
             payload_batch(6, 120, True, 9602, ecc=coded, mod=2), encode_call, encode_right, tx_roles),
        Case("encode_host-fcs_rs255_k7f_r34-ragged-chunk4", ("ofdm_tx_encode_host",), dict(plain, modulation=2, ecc=coded),
             payload_batch(6, 120, True, 9602, ecc=coded, mod=2), encode_host_call, encode_right, tx_roles),
        Case("normalize", ("ofdm_normalize_batch",), plain, normalize_build, normalize_call, normalize_right, frozenset({"kWsFrameMax"})),
        Case("encode_batch_sc16-two_pass-chunk4", ("ofdm_tx_encode_sc16_batch",), dict(plain, tuning={"no_txframe64_sc16": 1, "sc16_chunk_frames": 4}),
             payload_batch(6, 200, True, 9603), encode_sc16_call(sc), encode_sc16_right(sc), frozenset({"kWsTxSc16"})),
        Case("encode_host_sc16-two_pass-chunk4", ("ofdm_tx_encode_sc16_host",), dict(plain, tuning={"no_txframe64_sc16": 1, "sc16_chunk_frames": 3}),
             payload_batch(6, 200, True, 9603), encode_host_sc16_call(sc), encode_sc16_right(sc), frozenset({"kWsTxSc16"})),
    ]


# ---------------------------------------------------------------------------------------------------------------- stages
def chest_build(api, big):
    """five rows (ten: big) of LS estimates of the seeded link's frames, and the bare H = 1"""
    inp = std_batch(api, kinds=("whole",) * 4, big=big, seed=9700)
    maker = api.Context(n_fft=64, modulation=4, guard_bands=True)
    r = maker.decode_batch(inp["rx"], inp["D"])
    hk = maker.estimate_channel(inp["rx"], r["offset"], r["f_delta"]).cpu().numpy()
    rows = np.concatenate([hk, np.ones((2 if big else 1, 64), np.complex64)])
    return {"hk_np": rows, "rx": inp["rx"], "offset": r["offset"], "f_delta": r["f_delta"]}


def chest_call(ctx, inp):
    return arrays(ctx, hk=ctx.chest_smooth(ctx.to_device(inp["hk_np"])))


def chest_right(api, orc, inp, out):
    """tests/test_gpu_chest.py's bar: within max(4 x the complex64 restatement's own error, 1e-5) of the f64 definition"""
    import chest_ref as cr

    trn = orc.default_training(64)
    want = cr.smooth(inp["hk_np"].astype(np.complex128), trn, 64)
    c64 = cr.smooth_c64(inp["hk_np"], trn, 64)
    tol = max(4.0 * max(rel_err(c64[r], want[r]) for r in range(len(want))), 1e-5)
    err = max(rel_err(out["hk"][r], want[r]) for r in range(len(want)))
    assert err <= tol, (err, tol)


def chest_wls_call(ctx, inp):
    """ofdm_estimate_channel_batch under chest_mode = OFDM_CHEST_WLS: the LS estimate denoised in place"""
    return arrays(ctx, hk=ctx.estimate_channel(inp["rx"], inp["offset"], inp["f_delta"]))


def chest_wls_right(api, orc, inp, out):
    n = out["hk"].shape[0]
    chest_right(api, orc, {"hk_np": inp["hk_np"][:n]}, out)


def xcorr_call(ctx, inp):
    idx, pk = ctx.xcorr(inp["rx"], ctx.to_device(inp["lock"]))
    return arrays(ctx, idx_max=idx, peak=pk)


def xcorr_build(api, big):
    from oracle import oracle as orc

    inp = search_batch(64, 4, 200)(api, big)
    inp["lock"] = np.asarray(orc.locking_signal(80)).astype(np.complex64)
    return inp


def xcorr_right(api, orc, inp, out):
    """SignalRef::xcorr_fft's index of the f64 oracle (tests/test_gpu_gain.py), on the rows that hold a frame"""
    for f, row in enumerate(inp["rx_np"][:-1]):
        assert int(out["idx_max"][f]) == orc.xcorr_fft(row.astype(np.complex128), orc.locking_signal(80))[0], f


def cfo_wide_build(api, big):
    import torch
    from tools.link import wide_link_on

    maker = api.Context(n_fft=64, modulation=2, guard_bands=True)
    pay, rx, m, fd = wide_link_on(maker, 10 if big else 5, 120, 25.0, 9800)
    d, fsc, _ = maker.sc_correlate(rx)
    off = torch.clamp(d - maker.S - 4, min=0).to(torch.int32)
    maker.synchronize()
    return {"rx": rx, "offset": off, "f_sc": fsc, "m": m.cpu().numpy(), "fd": fd.cpu().numpy(), "rx_np": rx.cpu().numpy(),
            "off_np": off.cpu().numpy(), "f_sc_np": fsc.cpu().numpy()}


def cfo_wide_call(ctx, inp):
    r = ctx.cfo_wide(inp["rx"], inp["offset"], inp["f_sc"])
    return arrays(ctx, m=r["m"], f_delta=r["f_delta"], metric=r["metric"])


def cfo_wide_right(api, orc, inp, out):
    """tests/test_gpu_cfo_wide.py's bars: m and f0 + 2 pi m / S of the f64 definition (tests/cfo_wide_ref.py) exactly, the metrics within
    max(4 x the complex64 restatement's own distance, 1e-5); the definition finds the multiples the link was built with, and the total
    is within 0.05 sub-carrier spacings of what the channel turned by"""
    import test_gpu_cfo_wide as T

    k = dict(rx=inp["rx_np"], trn=orc.default_training(64), off=inp["off_np"], f0=inp["f_sc_np"])
    m, fd, g, tol, _, live = T._reference(k, 64, 8)
    assert live.all() and np.array_equal(m, inp["m"])
    assert np.array_equal(out["m"], m) and out["f_delta"].tobytes() == fd.tobytes()
    assert np.all(np.abs(out["metric"].astype(np.float64) - g) <= tol * np.abs(g))
    assert np.max(np.abs(out["f_delta"] - inp["fd"])) <= 0.05 * 2.0 * np.pi / 80


def llrw_build(api, big):
    """tests/test_gpu_noise_weight.py's stage case (N = 64, 64-QAM, rows of 7 symbols at 14 dB through a channel a row), with the weights
    k_noise_bins measures on as many rows of the seeded link"""
    import soft_ref as sr
    from oracle import oracle as orc
    from util import fc32, make_symbols_np

    n, mod, D, F = 64, 6, 7, 10 if big else 5
    rng = np.random.default_rng(9900 + big)
    hk = fc32(1.0 + 0.3 * (rng.standard_normal((F, n)) + 1j * rng.standard_normal((F, n))))
    x, _ = make_symbols_np(orc, rng, F * D, n, True, mod, snr_db=14.0)
    x = sr.through_h(x.reshape(F, -1), n, hk)
    link = std_batch(api, mod=2, ecc=0, payload=120, snr=20.0, kinds=("whole",) * 5, big=big, seed=9901)
    maker = api.Context(n_fft=n, modulation=2, guard_bands=True)
    r = maker.decode_batch(link["rx"], link["D"])
    nb = maker.noise_bins(link["rx"], r["offset"], r["f_delta"], r["status"])
    maker.synchronize()
    return {"x": maker.to_device(x), "x_np": x, "hk": maker.to_device(hk), "hk_np": hk, "q": nb["weight"].contiguous(), "D": D, "mod": mod,
            "nb": {k: v.cpu().numpy() for k, v in nb.items()}, "link_np": link["rx"].cpu().numpy(),
            "link_at": {k: r[k].cpu().numpy() for k in ("offset", "f_delta", "status")}}


def llrw_call(ctx, inp):
    return arrays(ctx, llr=ctx.rx_llr(inp["x"], inp["D"], hk=inp["hk"], bin_weight=inp["q"]))


def llrw_right(api, orc, inp, out):
    """tests/test_gpu_noise_weight.py's bars: the weights within S_TOL of tests/noise_weight_ref.py, and the LLRs by soft_ref.llr_compare
    against the f64 oracle's LLRs times q, at most 2 % of them excused"""
    import noise_weight_ref as nw
    import soft_ref as sr
    from test_gpu_noise_weight import S_TOL

    at = inp["link_at"]
    assert (at["status"] == 0).all()
    ws, wq = nw.noise_bins(inp["link_np"].astype(np.complex128), 64, at["offset"], at["f_delta"], at["status"])
    s, q = inp["nb"]["nvar"].astype(np.float64), inp["nb"]["weight"].astype(np.float64)
    assert max(np.linalg.norm(s[f] - ws[f]) / np.linalg.norm(ws[f]) for f in range(len(ws))) <= S_TOL and np.abs(q - wq).max() <= S_TOL
    assert (q < 1).any() and (q > 0).all()
    F, D, mod = inp["x_np"].shape[0], inp["D"], inp["mod"]
    ref = sr.oracle_llr_reference(orc, inp["x_np"], 64, True, mod, 32.0, inp["hk_np"])
    bins = sr.data_bins(orc, 64, True)
    qw = q[:, bins][:, None, :, None]
    shape = (F, D, bins.size, mod)
    y = (ref["y"].reshape(shape) * qw).reshape(F, -1)
    eps = (ref["eps"].reshape(shape) * qw).reshape(F, -1) + np.abs(y) * 2.0 ** -24    # one more f32 rounding: the product with q
    assert sr.llr_compare(out["llr"], y, eps, what="rx_llr_weighted") <= 0.02


def viterbi_build(rate):
    def build(api, big):
        import torch

        maker = api.Context(n_fft=64, modulation=2, guard_bands=True)
        rng = np.random.default_rng(9950)
        nf, nb = (12, 150) if big else (6, 97)
        pay = rng.integers(0, 256, (nf, nb), dtype=np.uint8)
        code = maker.conv_encode(maker.to_device(pay), rate=rate).cpu().numpy()
        n_steps = 8 * (nb + 1)
        bits = np.unpackbits(code, axis=1, bitorder="little")
        kept = bits.shape[1] if rate is None else int(maker.lib.ofdm_conv_k7_kept_bits(n_steps, rate))
        llr = np.where(bits[:, :kept] == 1, 90, -90).astype(np.int8)
        flip = rng.random(llr.shape) < 0.02                # a few wrong, weak LLRs: the decoder has something to do
        llr[flip] = (-llr[flip] // 6).astype(np.int8)
        return {"llr": torch.from_numpy(np.ascontiguousarray(llr)).to(maker.device), "pay": pay, "n_steps": n_steps, "rate": rate}
    return build


def viterbi_call(ctx, inp):
    return arrays(ctx, bytes=ctx.viterbi_decode_soft(inp["llr"], n_steps=inp["n_steps"], rate=inp["rate"]))


def viterbi_right(api, orc, inp, out):
    assert np.array_equal(out["bytes"][:, : inp["pay"].shape[1]], inp["pay"]) and (out["bytes"][:, inp["pay"].shape[1]:] == 0).all()


def stage_cases():
    c = dict(n_fft=64, modulation=4, guard_bands=True)
    q = dict(n_fft=64, modulation=2, guard_bands=True)
    return [
        Case("chest_smooth", ("ofdm_chest_smooth_batch",), c, chest_build, chest_call, chest_right, frozenset({"kWsChestTaps"})),
        Case("estimate_channel-chest_wls", ("ofdm_estimate_channel_batch",), dict(c, chest_mode=A.CHEST_WLS), chest_build, chest_wls_call, chest_wls_right,
             frozenset({"kWsChestTaps"})),
        Case("xcorr", ("ofdm_xcorr_batch",), c, xcorr_build, xcorr_call, xcorr_right, frozenset({"kWsSearch"})),
        Case("cfo_wide", ("ofdm_cfo_wide_batch",), q, cfo_wide_build, cfo_wide_call, cfo_wide_right, frozenset()),
        Case("rx_llr_weighted-noise_bins", ("ofdm_rx_llr_weighted_batch",), dict(q, modulation=6), llrw_build, llrw_call, llrw_right, frozenset()),
        Case("conv_k7_decode_soft", ("ofdm_conv_k7_decode_soft",), q, viterbi_build(None), viterbi_call, viterbi_right, frozenset({"kWsSurvivors"})),
        Case("conv_k7_decode_punctured-r34", ("ofdm_conv_k7_decode_punctured",), q, viterbi_build(A.CONV_RATE_3_4), viterbi_call, viterbi_right,
             frozenset({"kWsSurvivors"})),
    ]


# ---------------------------------------------------------------------------------------------------------------- one long capture
GAPS = (0, 37, 402, 3, 1211)                               # samples of silence in front of packet k (the link's own 1 .. 32 come on top)


def long_build(api, big):
    """five packets (ten: big) of the seeded link back to back with unequal gaps, the last cut by the capture's end; the maker's own scan of
    it (what decode_packets is handed), the capture on the device, on the host and quantised to sc16"""
    import torch
    from tools.link import link_on

    import sc16_ref

    maker = api.Context(n_fft=64, modulation=4, guard_bands=True)
    nf = 10 if big else 5
    pay, rx = link_on(maker, nf, 200, 30.0, 9990)
    span, S = rx.shape[1], maker.S
    at, pos = [], 0
    for f in range(nf):
        pos += GAPS[f % len(GAPS)]
        at.append(pos)
        pos += span
    cap = torch.zeros(pos, dtype=torch.complex64, device=maker.device)
    for f, st in enumerate(at):
        cap[st: st + span] = rx[f]
    end = (at[-1] + span - 160 - 2 * S - 5) & ~1           # the last packet loses its last data symbols
    cap = cap[:end].contiguous()
    D = maker.data_symbols(200)
    holdoff = maker.frame_samples(200) - 3 * S
    det = maker.sc_scan_long(cap, holdoff, ALL)
    assert det["d_hat"].size == nf and not det["more"], det
    maker.synchronize()
    cap_np = cap.cpu().numpy()
    q, scale = sc16_ref.quantise(cap_np, 0.9)
    return {"cap": cap, "cap_np": cap_np, "q_np": np.ascontiguousarray(q), "q": torch.from_numpy(np.ascontiguousarray(q)).to(maker.device),
            "scale": float(scale), "at": at, "pay": pay.cpu().numpy(), "det": det, "holdoff": holdoff, "D": D * (2 if big else 1), "payload": 200,
            "lag_lo3": int(det["lag_lo"][3]), "nf": nf}


def _packet_is(out, row, inp, k, cut=False):
    st, ln, p = int(out["status"][row]), int(out["len"][row]), inp["payload"]
    if not cut:
        assert st == 0 and ln == p and bytes(out["bytes"][row, :p]) == bytes(inp["pay"][k]), (k, st, ln)
    else:                                                  # cut by the capture's end: the whole symbols' bytes (the last live one is the zero-padded tail chunk)
        whole = (inp["cap"].numel() - int(out["offset"][row]) - 10 * 80) // 80
        n_cmp = min(ln, whole * 24 - 16)
        assert st == 0 and 0 < n_cmp <= ln < p and bytes(out["bytes"][row, :n_cmp]) == bytes(inp["pay"][k, :n_cmp]), (k, st, ln, n_cmp)
    lo = inp["at"][k]
    assert lo <= int(out["offset"][row]) <= lo + 40, (k, int(out["offset"][row]), lo)      # the link's delay of 1 .. 32 and the 5 samples behind the back-off


def long_decode_right(k):
    return lambda api, orc, inp, out: _packet_is(out, 0, inp, k)


def scan_reference(orc, inp):
    """tests/scan_ref.py's definition of the capture's scan, computed once per capture"""
    import scan_ref as R

    if "scan_ref" not in inp:
        inp["scan_ref"] = R.scan(orc, inp["cap_np"], 80, 3, 0.5, inp["holdoff"], ALL)
    return inp["scan_ref"]


def scan_right(api, orc, inp, out):
    """tests/test_gpu_scan.py's bar (same_as_reference): d1, d_hat, lag_lo and more of tests/scan_ref.py exactly, f_delta within 1e-9,
    metric within 1e-6; and the capture holds every packet once"""
    from test_gpu_scan import same_as_reference

    want = scan_reference(orc, inp)
    assert len(want.d1) == inp["nf"] == out["n"][0]
    same_as_reference({k: out[k] for k in ("d1", "d_hat", "lag_lo", "f_delta", "metric")} | {"more": bool(out["more"][0])}, want, "scan")


def scan_out(ctx, r):
    return arrays(ctx, n=np.int64(r["d_hat"].size), more=np.int32(r["more"]), d1=r["d1"], d_hat=r["d_hat"], f_delta=r["f_delta"], metric=r["metric"],
                  lag_lo=r["lag_lo"], next_lag_lo=np.int64(r["next_lag_lo"]))


def packets_reference(orc, inp, out, det, big=False):
    """tests/test_gpu_packets.py's bar: status, offset and out_len of tests/packets_ref.py exactly, the bytes under util.assert_bytes_match
    with the oracle's soft points (offset: only where the call delivers it)"""
    import packets_ref as P
    from util import assert_bytes_match

    want = P.packets(orc, inp["cap_np"], det, 64, True, 4, inp["D"])
    for k, w in enumerate(want):
        assert (int(out["status"][k]), int(out["len"][k])) == (w["status"], w["len"]), (k, w["status"], w["len"])
        assert "offset" not in out or int(out["offset"][k]) == w["offset"], (k, w["offset"])
        if w["status"] == 0:
            assert_bytes_match(bytes(out["bytes"][k, : w["len"]]), w["bytes"], w["soft"][128 // 4:], 4, what=str(k))


def packets_right(api, orc, inp, out):
    det = inp["det"] if "d_hat" not in out else {k: out[k] for k in ("d_hat", "f_delta", "metric")}
    if "d_hat" in out:                                     # decode_all_host: its own scan first
        from test_gpu_scan import same_as_reference

        want = scan_reference(orc, inp)
        got = {"d1": out["d1"], "d_hat": out["d_hat"], "lag_lo": np.concatenate([[0], out["d1"][:-1] + inp["holdoff"]]), "f_delta": det["f_delta"],
               "metric": det["metric"], "more": bool(out["more"][0])}
        same_as_reference(got, want, "decode_all_host")
    packets_reference(orc, inp, out, det)
    for k in range(inp["nf"]):
        _packet_is(out, k, inp, k, cut=k == inp["nf"] - 1)
    assert out["f_delta"].tobytes() == np.asarray(det["f_delta"]).tobytes()                # CFO_SIGNED: what the chain derotated with
    assert out["metric"].tobytes() == np.asarray(det["metric"]).tobytes()                  # the scan's, bit for bit (include/ofdm_hip.h)


def packets_bare_call(ctx, inp):
    """ofdm_rx_decode_packets without its optional outputs offset, f_delta and metric: the chain's f_delta lives in kWsPktFdelta"""
    import torch

    import rows as R

    det, p = inp["det"], R._p
    dh = np.ascontiguousarray(det["d_hat"], np.int64)
    fd = np.ascontiguousarray(det["f_delta"], np.float64)
    m = np.ascontiguousarray(det["metric"], np.float32)
    n, ob = dh.size, ctx.decode_row_bytes(inp["D"])
    res = {"bytes": ctx.empty((n, ob), torch.uint8), "len": ctx.empty((n,), torch.int32), "status": ctx.empty((n,), torch.int32)}
    rc = ctx.lib.ofdm_rx_decode_packets(ctx.h, p(inp["cap"]), inp["cap"].numel(), n, p(dh), p(fd), p(m), inp["D"], p(res["bytes"]), ob, p(res["len"]),
                                       p(res["status"]), None, None, None)
    assert rc == 0, rc
    ctx.synchronize()
    by = res["bytes"].cpu().numpy().copy()
    st, ln = res["status"].cpu().numpy(), res["len"].cpu().numpy()
    by[np.arange(ob)[None, :] >= np.where(st == 0, np.clip(ln, 0, ob), 0)[:, None]] = 0
    return {"status": st, "len": ln, "bytes": by}


def packets_bare_right(api, orc, inp, out):
    packets_reference(orc, inp, out, inp["det"])
    p = inp["payload"]
    for k in range(inp["nf"] - 1):
        assert int(out["status"][k]) == 0 and int(out["len"][k]) == p and bytes(out["bytes"][k, :p]) == bytes(inp["pay"][k]), k


def decode_all_call(ctx, inp):
    r = ctx.decode_all_host(inp["cap_np"], inp["holdoff"], ALL, inp["D"])
    out = rows_out(ctx, r)
    out.update(arrays(ctx, d1=r["d1"], d_hat=r["d_hat"], more=np.int32(r["more"])))
    return out                                             # (f_delta and metric: the packets' columns, which are the scan's)


def long_cases():
    c = dict(n_fft=64, modulation=4, guard_bands=True)
    SC64 = frozenset({"kWsSearch"})                        # the slice searches: rows of 2560 samples and less
    chain = FUSED64 | SC64
    pkt = frozenset({"kWsPktDet", "kWsPktGeom", "kWsPktRows", "kWsPktOffset", "kWsDhat", "kWsFdelta", "kWsOffset", "kWsNsym", "kWsRaw", "kWsCut"})
    scan = frozenset({"kWsScanBits", "kWsScanRows"})
    chunk2 = dict(c, tuning={"packets_chunk_rows": 2})

    def corr_right(api, orc, inp, out):
        assert int(out["d_hat"][0]) == int(inp["det"]["d_hat"][0]) and inp["at"][0] + 89 < int(out["d_hat"][0]) <= inp["at"][0] + 121
        wfd, wm = float(inp["det"]["f_delta"][0]), float(inp["det"]["metric"][0])      # the scan's, from other kernels: the search tests' bars
        assert abs(out["f_delta"][0] - wfd) <= 1e-9 and abs(out["metric"][0] - wm) <= 1e-6 * max(1.0, wm)

    def corr_call(ctx, inp):
        d, fd, m = ctx.sc_correlate_long(inp["cap"])
        return arrays(ctx, d_hat=np.int64(d), f_delta=np.float64(fd), metric=np.float32(m))

    return [
        Case("sc_correlate_long", ("ofdm_sc_correlate_long",), c, long_build, corr_call, corr_right, SC64),
        Case("decode_long-lag_lo_0", ("ofdm_rx_decode_long",), c, long_build, lambda ctx, inp: rows_out(ctx, ctx.decode_long(inp["cap"], inp["D"])),
             long_decode_right(0), chain),
        Case("decode_long-lag_lo_packet3", ("ofdm_rx_decode_long",), c, long_build,
             lambda ctx, inp: rows_out(ctx, ctx.decode_long(inp["cap"], inp["D"], lag_lo=inp["lag_lo3"])), long_decode_right(3), chain),
        Case("sc_scan_long", ("ofdm_sc_scan_long",), c, long_build, lambda ctx, inp: scan_out(ctx, ctx.sc_scan_long(inp["cap"], inp["holdoff"], ALL)),
             scan_right, scan),
        Case("decode_packets-chunk2", ("ofdm_rx_decode_packets",), chunk2, long_build,
             lambda ctx, inp: rows_out(ctx, ctx.decode_packets(inp["cap"], inp["det"], inp["D"])), packets_right, pkt),
        Case("decode_packets-chunk2-bare", ("ofdm_rx_decode_packets",), chunk2, long_build, packets_bare_call, packets_bare_right, pkt | {"kWsPktFdelta"}),
        Case("decode_long_sc16", ("ofdm_rx_decode_long_sc16",), c, long_build,
             lambda ctx, inp: rows_out(ctx, ctx.decode_long_sc16(inp["q"], inp["D"], scale=inp["scale"])), long_decode_right(0), chain | {"kWsLongSc16"}),
        Case("decode_long_host", ("ofdm_rx_decode_long_host",), c, long_build, lambda ctx, inp: rows_out(ctx, ctx.decode_long_host(inp["cap_np"], inp["D"])),
             long_decode_right(0), chain),
        Case("sc_scan_long_host", ("ofdm_sc_scan_long_host",), c, long_build,
             lambda ctx, inp: scan_out(ctx, ctx.sc_scan_long_host(inp["cap_np"], inp["holdoff"], ALL)), scan_right, scan),
        Case("decode_all_host-chunk2", ("ofdm_rx_decode_all_long_host",), chunk2, long_build, decode_all_call, packets_right, pkt | scan),
        Case("decode_long_host_sc16", ("ofdm_rx_decode_long_sc16_host",), c, long_build,
             lambda ctx, inp: rows_out(ctx, ctx.decode_long_host_sc16(inp["q_np"], inp["D"], scale=inp["scale"])), long_decode_right(0), chain | {"kWsLongSc16"}),
    ]


def all_cases():
    cases = decode_cases() + sc16_cases() + search_cases() + combine_cases() + transmit_cases() + stage_cases() + long_cases()
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = all_cases()

# The one call that takes a workspace and has no answer to compare: a read-only pass that sinks what it read
NO_ANSWER = {"ofdm_hbm_read_probe": "kWsProbeSink: a measurement pass, nothing is delivered"}

# Entry points that take no workspace and no pipe buffer, each with the reason (read off its body in ofdm_abi.hip) and the smallest valid
# call through ofdm_amd/api.py: tests/test_gpu_ws_poison.py runs each on a new context and finds stat_ws_live == 0
def _t(ctx, a, dtype=None):
    import torch

    return torch.as_tensor(np.asarray(a), dtype=dtype).to(ctx.device)


def _frame(ctx, n=1):
    import torch

    return ctx.encode_batch(torch.zeros((n, 8), dtype=torch.uint8, device=ctx.device))


def _i8(ctx, n):
    import torch

    return torch.full((1, n), 50, dtype=torch.int8, device=ctx.device)


def _raw(name, *args):
    return lambda ctx: ctx._ck(getattr(ctx.lib, name)(ctx.h, *args), name)


def _alloc_free(ctx):
    import ctypes as C

    p = C.c_void_p()
    ctx._ck(ctx.lib.ofdm_dev_alloc(ctx.h, 64, C.byref(p)), "dev_alloc")
    host = (C.c_uint8 * 64)()
    ctx._ck(ctx.lib.ofdm_memset(ctx.h, p, 7, 64), "memset")
    ctx._ck(ctx.lib.ofdm_memcpy_h2d(ctx.h, p, host, 16), "h2d")
    ctx._ck(ctx.lib.ofdm_memcpy_d2h(ctx.h, host, p, 64), "d2h")
    assert host[63] == 7 and host[0] == 0
    ctx._ck(ctx.lib.ofdm_dev_free(ctx.h, p), "dev_free")


def _set_stream(ctx):
    import torch

    ctx._ck(ctx.lib.ofdm_set_stream(ctx.h, torch.cuda.current_stream(ctx.device).cuda_stream), "set_stream")


STATE = "context state and queries: no launch"
ONE = "one launch into the caller's buffers"
NO_WORKSPACE = {
    # name: (reason, call)
    "ofdm_destroy": (STATE, lambda ctx: None),             # (the context's own close() at the end of the test)
    "ofdm_set_stream": (STATE, _set_stream),
    "ofdm_use_own_stream": (STATE, lambda ctx: ctx.use_own_stream()),
    "ofdm_synchronize": (STATE, lambda ctx: ctx.synchronize()),
    "ofdm_last_hip_error": (STATE, lambda ctx: ctx.lib.ofdm_last_hip_error(ctx.h)),
    "ofdm_last_dispatch": (STATE, lambda ctx: ctx.last_dispatch()),
    "ofdm_set_tuning": (STATE, lambda ctx: ctx.set_tuning("grid_cap", 0)),
    "ofdm_get_tuning": (STATE, lambda ctx: ctx.get_tuning("grid_cap")),
    "ofdm_set_llr_weight": (STATE, lambda ctx: ctx.set_llr_weight(0)),
    "ofdm_get_llr_weight": (STATE, lambda ctx: ctx.get_llr_weight()),
    "ofdm_dev_alloc": ("the caller's own allocation", _alloc_free),
    "ofdm_dev_free": ("the caller's own allocation", _alloc_free),
    "ofdm_memcpy_h2d": ("a copy", _alloc_free),
    "ofdm_memcpy_d2h": ("a copy", _alloc_free),
    "ofdm_memset": ("a fill of the caller's buffer", _alloc_free),
    "ofdm_symbol_len": (STATE, lambda ctx: ctx.lib.ofdm_symbol_len(ctx.h)),
    "ofdm_data_carriers": (STATE, lambda ctx: ctx.lib.ofdm_data_carriers(ctx.h)),
    "ofdm_bytes_per_symbol": (STATE, lambda ctx: ctx.lib.ofdm_bytes_per_symbol(ctx.h)),
    "ofdm_coded_len": (STATE, lambda ctx: ctx.coded_len(8)),
    "ofdm_data_symbols": (STATE, lambda ctx: ctx.data_symbols(8)),
    "ofdm_frame_samples": (STATE, lambda ctx: ctx.frame_samples(8)),
    "ofdm_chest_window": (STATE, lambda ctx: ctx.chest_window()),
    "ofdm_timer_start": ("an event record", lambda ctx: ctx.timer_start()),
    "ofdm_timer_stop_ms": ("an event record", lambda ctx: (ctx.timer_start(), ctx.timer_stop_ms())),
    "ofdm_fft_batch": (ONE, lambda ctx: ctx.fft(_t(ctx, np.ones((1, 64), np.complex64)))),
    "ofdm_ifft_cp_batch": (ONE, lambda ctx: ctx.prefix_block(_t(ctx, np.ones((1, 64), np.complex64)))),
    "ofdm_tx_symbols_batch": (ONE, lambda ctx: ctx.tx_symbols(_t(ctx, np.zeros(ctx.bytes_per_symbol, np.uint8)), 1)),
    "ofdm_unprefix_batch": (ONE, lambda ctx: ctx.unprefix_block(_t(ctx, np.ones((1, 80), np.complex64)))),
    "ofdm_qam_map_batch": (ONE, lambda ctx: ctx.modulate(_t(ctx, np.zeros(8, np.uint8)))),
    "ofdm_qam_demap_batch": (ONE, lambda ctx: ctx.demodulate(ctx.modulate(_t(ctx, np.zeros(8, np.uint8))))),
    "ofdm_encode_block_batch": (ONE, lambda ctx: ctx.encode_block(_t(ctx, np.ones((1, ctx.data_carriers), np.complex64)))),
    "ofdm_hamming74_encode": (ONE, lambda ctx: ctx.hamming74_encode(_t(ctx, np.zeros(4, np.uint8)))),
    "ofdm_hamming74_decode": (ONE, lambda ctx: ctx.hamming74_decode(_t(ctx, np.zeros(7, np.uint8)))),
    "ofdm_hamming74_decode_soft": (ONE, lambda ctx: ctx.hamming74_decode_soft(_i8(ctx, 56).reshape(-1))),
    "ofdm_frequency_correction_batch": (ONE, lambda ctx: ctx.frequency_correction(_t(ctx, np.ones((1, 160), np.complex64)))),
    "ofdm_cfo_rotate_batch": (ONE, lambda ctx: ctx.cfo_rotate(_t(ctx, np.ones((1, 80), np.complex64)), _t(ctx, np.zeros(1, np.float64)))),
    "ofdm_rx_demod_batch": ("the caller's rows in, the caller's rows out (every N: k_demod64, k_demod_mid, k_demod4096, k_sym<demod>)",
                            lambda ctx: ctx.rx_demod(_frame(ctx)[:, 800:].contiguous(), 1)),
    "ofdm_rx_llr_batch": (ONE, lambda ctx: ctx.rx_llr(_frame(ctx)[:, 800:].contiguous(), 1)),
    "ofdm_rx_quality_batch": (ONE, lambda ctx: ctx.rx_quality(_frame(ctx), 1)),
    "ofdm_rx_noise_bins_batch": (ONE, lambda ctx: ctx.noise_bins(_frame(ctx), _t(ctx, np.zeros(1, np.int32)))),
    "ofdm_conv_k7_encode": (ONE, lambda ctx: ctx.conv_encode(_t(ctx, np.zeros((1, 4), np.uint8)))),
    "ofdm_conv_k7_encode_punctured": (ONE, lambda ctx: ctx.conv_encode(_t(ctx, np.zeros((1, 4), np.uint8)), rate=1)),
    "ofdm_rs255_encode_batch": (ONE, lambda ctx: ctx.rs255_encode(_t(ctx, np.zeros((1, 8), np.uint8)))),
    "ofdm_rs255_decode_batch": (ONE, lambda ctx: ctx.rs255_decode(ctx.rs255_encode(_t(ctx, np.zeros((1, 8), np.uint8))))),
    "ofdm_ldpc648_encode_batch": (ONE, lambda ctx: ctx.ldpc_encode(_t(ctx, np.zeros((1, 40), np.uint8)))),
    "ofdm_ldpc648_decode_batch": (ONE, lambda ctx: ctx.ldpc_decode(_i8(ctx, 640))),
    "ofdm_ldpc648_encode_rate_batch": (ONE, lambda ctx: ctx.ldpc_encode(_t(ctx, np.zeros((1, 53), np.uint8)), rate=1)),
    "ofdm_ldpc648_decode_rate_batch": (ONE, lambda ctx: ctx.ldpc_decode(_i8(ctx, 640), rate=1)),
    "ofdm_fcs_wrap_batch": (ONE, lambda ctx: ctx.fcs_wrap(_t(ctx, np.zeros((1, 8), np.uint8)))),
    "ofdm_fcs_check_batch": (ONE, lambda ctx: ctx.fcs_check(ctx.fcs_wrap(_t(ctx, np.zeros((1, 8), np.uint8))))),
    "ofdm_llr_combine_batch": (ONE, lambda ctx: ctx.llr_combine(_i8(ctx, 64).repeat(2, 1), 2)),
    "ofdm_sc16_widen_batch": (ONE, lambda ctx: ctx.sc16_widen(_t(ctx, np.ones((1, 8, 2), np.int16)))),
    "ofdm_sc16_narrow_batch": (ONE, lambda ctx: ctx.sc16_narrow(_t(ctx, np.ones((1, 8), np.complex64)))),
    "ofdm_channel_batch": (ONE, lambda ctx: ctx.channel_batch(_frame(ctx))),
}
