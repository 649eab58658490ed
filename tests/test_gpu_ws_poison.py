"""No entry point's answer may depend on what the context's workspaces, or the host pipe's device and pinned buffers, held before the
call ("the workspace ledger").  The buffers are grown on demand, never cleared and handed from call to call for the life of
the context; a kernel that reads one element more than a kernel of the same call wrote is right on a new context, whose allocations
usually read as zeros, and wrong on a used one.  The laboratory key ws_poison (ofdm_amd/csrc/ofdm_hip_tuning.h) fills every buffer the
context holds, and every later growth, with a byte of the test's choosing; one rule is applied to every case of tests/ws_cases.py:

  1. premise      two new contexts give the same outputs bit for bit and the same last_dispatch() (run-to-run differences are not
                  staleness), and the answer is right by the bar the entry point's own test file uses;
  2. fresh growth a third new context, armed with 0x1FF before its first call so that every growth is filled: the premise's outputs
                  and dispatch string, and stat_ws_live is exactly the roles the case declares;
  3. re-arm       armed again with 0x17F, 0x100 and 0x1FF, a call after each: 0xFF is NaN as a float, -1 as an integer and every bit
                  of a bitmap; 0x7F is +127 as an LLR, 3.4e38 as a float and a large count; 0x00 is what a new allocation looks like;
  4. history      on the same context, still armed, the big variant (twice the rows, a larger max_symbols): the workspaces that hold rows
                  (kWsRaw, kWsHk, kWsLlr: asserted) are freed and allocated again in mid-life -- the per-frame arrays fit the slack of
                  their first allocation and stay --, and the answer is a new context's; then the original call again.

No tolerance is new: everything between contexts is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import ws_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(ofdm):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ofdm_amd import api as _api

    return _api


@functools.lru_cache(maxsize=None)
def _built(api, build, big):
    return build(api, big)


def inputs(api, case, big):
    """the case's inputs, built once on a maker context of their own and shared by every context under test"""
    return _built(api, case.build, big)


def fresh(api, case, poison=None):
    ctx = api.Context(**case.ctx)
    if poison is not None:
        ctx.set_tuning("ws_poison", poison)
        assert ctx.get_tuning("ws_poison") == poison and ctx.get_tuning("stat_ws_live") == 0
    return ctx


def run(case, ctx, inp, close=False):
    out = case.call(ctx, inp)
    ctx.synchronize()
    disp = ctx.last_dispatch()
    if close:
        ctx.close()
    return out, disp


ROW_ROLES = ("kWsRaw", "kWsHk", "kWsLlr")                  # rows of a frame each: twice the rows of more symbols outgrow bytes / 8 + 256 of slack


def caps(ctx, names):
    order = W.ws_roles()
    return {n: (ctx.get_tuning(f"stat_ws_ptr:{order.index(n)}"), ctx.get_tuning(f"stat_ws_cap:{order.index(n)}")) for n in names}


def assert_same(case, got, want, what):
    (out, disp), (wout, wdisp) = got, want
    field = W.same(out, wout)
    if field is not None and field in out and field in wout and out[field].shape == wout[field].shape:
        bad = np.flatnonzero(out[field].reshape(-1).view(np.uint8) != wout[field].reshape(-1).view(np.uint8))
        raise AssertionError(f"{case.id}, {what}: '{field}' differs at {bad.size} bytes, first at byte {int(bad[0])} of {out[field].shape} {out[field].dtype}")
    assert field is None, (case.id, what, field)
    assert disp == wdisp, (case.id, what, disp, wdisp)


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_answer_does_not_depend_on_what_the_workspaces_held(api, orc, case):
    inp = inputs(api, case, False)
    # 1. the premise
    premise = run(case, fresh(api, case), inp, close=True)
    assert_same(case, run(case, fresh(api, case), inp, close=True), premise, "two new contexts")
    case.right(api, orc, inp, premise[0])
    # 2. every growth poisoned
    ctx = fresh(api, case, 0x1FF)
    assert_same(case, run(case, ctx, inp), premise, "first call, every growth filled with 0xFF")
    live = ctx.get_tuning("stat_ws_live")
    assert W.mask_names(live) == sorted(case.roles), (case.id, "roles held", W.mask_names(live), "declared", sorted(case.roles))
    # 3. everything the context holds poisoned again
    for fill in (0x17F, 0x100, 0x1FF):
        ctx.set_tuning("ws_poison", fill)
        assert_same(case, run(case, ctx, inp), premise, f"re-armed with {fill & 0xFF:#04x}")
    # 4. a larger call in mid-life, then the original one
    big = inputs(api, case, True)
    grows = [n for n in ROW_ROLES if n in case.roles] if case.id.startswith(("decode_batch", "decode_host", "decode_combine")) else []
    before = caps(ctx, grows)
    assert_same(case, run(case, ctx, big), run(case, fresh(api, case), big, close=True), "the big variant on the used context")
    assert ctx.get_tuning("stat_ws_live") == live
    for n, (ptr, cap) in caps(ctx, grows).items():         # a free and a new, poisoned allocation in mid-life
        assert cap > before[n][1], (case.id, n, before[n], (ptr, cap))
    ctx.set_tuning("ws_poison", 0x1FF)
    assert_same(case, run(case, ctx, inp), premise, "the original call after the big one")
    ctx.close()


def _read_role(ctx, r):
    ptr, cap = ctx.get_tuning(f"stat_ws_ptr:{r}"), ctx.get_tuning(f"stat_ws_cap:{r}")
    if not ptr:
        assert cap == 0
        return None
    buf = (C.c_uint8 * cap)()
    ctx._ck(ctx.lib.ofdm_memcpy_d2h(ctx.h, buf, C.c_void_p(ptr), cap), "memcpy_d2h")
    return np.frombuffer(buf, np.uint8)


def _read_pipe(ctx, i):
    ptr, cap, pinned = (ctx.get_tuning(f"stat_pipe_{k}:{i}") for k in ("ptr", "cap", "pinned"))
    if not ptr:
        assert cap == 0
        return None
    if pinned:
        return np.frombuffer(C.string_at(ptr, cap), np.uint8)
    buf = (C.c_uint8 * cap)()
    ctx._ck(ctx.lib.ofdm_memcpy_d2h(ctx.h, buf, C.c_void_p(ptr), cap), "memcpy_d2h")
    return np.frombuffer(buf, np.uint8)


def _case(cid):
    return next(c for c in W.CASES if c.id == cid)


def test_arming_reaches_every_byte_of_every_live_role(api):
    """after a decode through the host pipe (every role of the fused chain, three device and three pinned slots): ws_poison = 0x1EE, then
    every live role read back whole through stat_ws_ptr / stat_ws_cap holds 0xEE alone; a role that holds nothing reports 0 / 0"""
    case = _case("decode_host-none-chunk4")
    ctx = fresh(api, case)
    run(case, ctx, inputs(api, case, False))
    roles = W.ws_roles()
    assert ctx.get_tuning("stat_ws_roles") == len(roles)
    live = ctx.get_tuning("stat_ws_live")
    assert W.mask_names(live) == sorted(case.roles)
    ctx.set_tuning("ws_poison", 0x1EE)
    for r, name in enumerate(roles):
        got = _read_role(ctx, r)
        assert (got is not None) == bool(live >> r & 1), name
        if got is not None:
            assert got.size >= 256 and (got == 0xEE).all(), (name, got.size, int((got != 0xEE).sum()))
    ctx.close()


def test_arming_and_growth_reach_every_buffer_of_the_host_pipe(api):
    """the pipe's 16 buffers through stat_pipe_*: none before the first host call; after the chunked decode, the long decodes (fc32 and sc16)
    and the scan from pageable memory every one of them holds memory; armed with 0x1EE all of them hold 0xEE alone.  Then a context armed
    BEFORE its first host call: the 64 bytes and more of slack behind what every dev_grow / pin_grow was asked for still hold the fill"""
    dec, lng = _case("decode_host-none-chunk4"), _case("decode_long_host")
    scan, lng16 = _case("sc_scan_long_host"), _case("decode_long_host_sc16")
    for armed_first in (False, True):
        ctx = fresh(api, dec, 0x1AB if armed_first else None)
        n = ctx.get_tuning("stat_pipe_bufs")
        assert n == 16 and all(_read_pipe(ctx, i) is None for i in range(n))
        d = inputs(api, dec, False)
        ctx.decode_host(d["rx_np"], d["D"], chunk_frames=2)   # three chunks: all three slots of every kind
        for case in (lng, scan, lng16):
            run(case, ctx, inputs(api, case, False))
        held = [_read_pipe(ctx, i) for i in range(n)]
        assert all(b is not None and b.size >= 256 for b in held), [i for i, b in enumerate(held) if b is None]
        assert sum(ctx.get_tuning(f"stat_pipe_pinned:{i}") for i in range(n)) == 7
        if armed_first:
            for i, b in enumerate(held):
                assert (b[-32:] == 0xAB).all(), i
        else:
            ctx.set_tuning("ws_poison", 0x1EE)
            for i in range(n):
                b = _read_pipe(ctx, i)
                assert (b == 0xEE).all(), (i, b.size, int((b != 0xEE).sum()))
        with pytest.raises(api.OfdmError):
            ctx.get_tuning(f"stat_pipe_ptr:{n}")
        ctx.close()


def test_growth_is_filled_while_the_key_is_on_and_left_alone_when_off(api):
    """armed before the first call: what a growth hands out is filled over its whole capacity -- the 256 bytes of slack behind what the
    call asked for (ws_get: bytes + bytes / 8 + 256) still hold the fill after the call.  Off again: the key reads 0 and the next call's
    answer is the same"""
    case = _case("decode_batch-fcs_ldpc648_r34")
    inp = inputs(api, case, False)
    ctx = fresh(api, case, 0x1AB)
    first = run(case, ctx, inp)
    live = ctx.get_tuning("stat_ws_live")
    assert live == W.role_mask(case.roles)
    for r, name in enumerate(W.ws_roles()):
        got = _read_role(ctx, r)
        if got is not None:
            assert (got[-128:] == 0xAB).all(), name
    ctx.set_tuning("ws_poison", 0)
    assert ctx.get_tuning("ws_poison") == 0
    assert_same(case, run(case, ctx, inp), first, "the key off again")
    ctx.close()


def test_the_key_takes_only_its_values(api):
    ctx = api.Context()
    for bad in (1, 0xFF, 0x200, -1, 0x1FF + 0x100, 1 << 40):
        with pytest.raises(api.OfdmError):
            ctx.set_tuning("ws_poison", bad)
    assert ctx.get_tuning("ws_poison") == 0
    for ok in (0x100, 0x1FF, 0x17F, 0):
        ctx.set_tuning("ws_poison", ok)
        assert ctx.get_tuning("ws_poison") == ok
    for bad in ("stat_ws_ptr:", "stat_ws_ptr:-1", f"stat_ws_cap:{len(W.ws_roles())}", "stat_ws_ptr:1x", "stat_ws_cap", "stat_ws_ptr: 3", "stat_ws_ptr:+3",
                "stat_pipe_ptr:", "stat_pipe_cap: 1", "stat_pipe_pinned:99"):
        with pytest.raises(api.OfdmError):
            ctx.get_tuning(bad)
    for key in ("stat_ws_roles", "stat_ws_live", "stat_ws_ptr:0"):       # read-only
        with pytest.raises(api.OfdmError):
            ctx.set_tuning(key, 0)


@pytest.mark.parametrize("name", sorted(W.NO_WORKSPACE))
def test_entry_points_without_a_workspace_hold_none(api, name):
    """the smallest valid call of every entry point the table leaves out, on a new context: no role holds memory afterwards"""
    ctx = api.Context(n_fft=64, modulation=api.QAM16, guard_bands=True)
    W.NO_WORKSPACE[name][1](ctx)
    ctx.synchronize()
    assert ctx.get_tuning("stat_ws_live") == 0, W.mask_names(ctx.get_tuning("stat_ws_live"))
    ctx.close()
