"""The table of tests/ws_cases.py is complete (no GPU): every workspace role of ofdm_amd/csrc/ofdm_ctx.hpp is one that a case must
touch, and every `ofdm_ctx *` entry point of include/ofdm_hip.h is a case's entry point or stands in NO_WORKSPACE with its reason.  A new
role or entry point without a case turns this red."""
import os
import re

import ws_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_role_is_touched_by_a_case():
    roles = W.ws_roles()
    assert len(roles) == len(set(roles)) >= 36 and roles[0] == "kWsDhat"
    declared = set().union(*[c.roles for c in W.CASES])
    assert declared <= set(roles), sorted(declared - set(roles))
    # kWsProbeSink: ofdm_hbm_read_probe's sink, a call without an answer (NO_ANSWER)
    assert set(roles) - declared == {"kWsProbeSink"}, sorted(set(roles) - declared)


def test_every_entry_point_is_a_case_or_has_a_reason():
    eps = set(W.ctx_entry_points())
    assert len(eps) >= 85 and {"ofdm_rx_decode_batch", "ofdm_get_tuning", "ofdm_timer_stop_ms", "ofdm_destroy"} <= eps
    cased = {e for c in W.CASES for e in c.entry}
    for listed in (cased, set(W.NO_WORKSPACE), set(W.NO_ANSWER)):
        assert listed <= eps, sorted(listed - eps)
    assert not (cased & set(W.NO_WORKSPACE)) and not (cased & set(W.NO_ANSWER)) and not (set(W.NO_WORKSPACE) & set(W.NO_ANSWER))
    assert eps == cased | set(W.NO_WORKSPACE) | set(W.NO_ANSWER), sorted(eps - cased - set(W.NO_WORKSPACE) - set(W.NO_ANSWER))
    assert set(W.NO_ANSWER) == {"ofdm_hbm_read_probe"}
    for name, (reason, call) in W.NO_WORKSPACE.items():
        assert reason.strip() and callable(call), name


def test_every_ws_get_names_a_role_some_case_declares():
    """the ws_get calls of the two translation units, by role (or by the table that holds the role): none is missing from the enum"""
    roles = set(W.ws_roles())
    src = "".join(open(os.path.join(ROOT, "ofdm_amd", "csrc", f)).read() for f in ("ofdm_abi.hip", "ofdm_host_path.hip"))
    named = set(re.findall(r"ws_get\(c, (kWs\w+),", src))
    assert named <= roles, sorted(named - roles)
    # the roles that reach ws_get through a table (the outer layers' rows and lengths) or an argument (the two sc16 chunk workspaces)
    indirect = set(re.findall(r"ws_get\(c, (?!kWs[A-Z])([a-zA-Z][\w.\[\]>-]*),", src))
    assert indirect == {"s.tx_rows", "s.tx_len", "role", "kOuter[m.outer[i]].rx_rows"}, indirect
    used = {r for r in roles if re.search(r"\b%s\b" % r, src)}
    assert used == roles, sorted(roles - used)             # a role nothing takes is dead: drop it from the enum


def test_cases_are_well_formed():
    ids = [c.id for c in W.CASES]
    assert len(ids) == len(set(ids))
    for c in W.CASES:
        assert c.entry and all(e.startswith("ofdm_") for e in c.entry), c.id
        assert callable(c.build) and callable(c.call) and callable(c.right), c.id
        assert isinstance(c.roles, frozenset), c.id
        assert set(c.ctx) <= {"n_fft", "modulation", "guard_bands", "ecc", "tuning", "chest_mode", "cfo_mode", "llr_weight", "sync_mode"}, c.id
    # every group of the table is there
    for want in ("decode_batch-none", "decode_batch-none-odd_out_stride", "decode_batch-hamming74_soft-chunk4", "decode_batch-n4096_none",
                 "sc_correlate-n128-tiles", "decode_combine-k7f_r12", "encode_batch-fcs_rs255_k7f_r34-ragged", "normalize",
                 "encode_batch_sc16-two_pass-chunk4", "decode_batch_sc16-none-chunk4", "rx_demod_sc16-widen-chunk4", "decode_long_sc16", "chest_smooth",
                 "xcorr", "cfo_wide", "rx_llr_weighted-noise_bins", "sc_correlate_long", "decode_long-lag_lo_0", "decode_long-lag_lo_packet3",
                 "sc_scan_long", "decode_packets-chunk2", "decode_packets-chunk2-bare", "decode_host-none-chunk4", "demod_host-chunk4",
                 "encode_host-fcs_rs255_k7f_r34-ragged-chunk4", "decode_long_host", "sc_scan_long_host", "decode_all_host-chunk2", "decode_long_host_sc16"):
        assert want in ids, want


def test_restated_constants_are_the_apis():
    """ws_cases.py restates a few constants of ofdm_amd/api.py so that it imports without torch"""
    import ast

    src = open(os.path.join(ROOT, "ofdm_amd", "api.py")).read()
    consts = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1:
            t, v = node.targets[0], node.value
            try:
                val = ast.literal_eval(v)
            except ValueError:
                continue
            if isinstance(t, ast.Name):
                consts[t.id] = val
            elif isinstance(t, ast.Tuple) and isinstance(val, tuple) and len(val) == len(t.elts):
                consts.update({e.id: x for e, x in zip(t.elts, val)})
    for name in dir(W.A):
        if name.isupper():
            assert consts[name] == getattr(W.A, name), name
    assert (W.FRAME_OK, W.FRAME_SHORT, W.FRAME_NOSYNC, W.FRAME_HEADER, W.FRAME_UNCORRECTABLE, W.FRAME_FCS) == tuple(
        consts[k] for k in ("FRAME_OK", "FRAME_SHORT", "FRAME_NOSYNC", "FRAME_HEADER", "FRAME_UNCORRECTABLE", "FRAME_FCS"))
