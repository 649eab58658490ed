"""numpy definition of EXT-7, soft combining (include/ofdm_hip.h "soft combining"): LLR-level (Chase) combining of R captures of one
frame, weighted by link quality, in exact integers.  Nothing in the reference corresponds to it (parity unpinned by the reference):
this file is the definition, and k_llr_combine (ofdm_amd/csrc/kernels_combine.hip) is compared with it bit for bit.

Layout: branch r of frame f is row f * R + r of every per-branch array."""
import numpy as np

MAX_BRANCHES = 8          # OFDM_COMBINE_MAX_BRANCHES
WEIGHT_ONE = 64           # OFDM_COMBINE_WEIGHT_ONE: the best live branch's weight
Q_VALID, Q_LLR_UNIT, QUALITY_FIELDS = 0, 4, 8   # OFDM_Q_VALID, OFDM_Q_LLR_UNIT, OFDM_QUALITY_FIELDS
HEADER_STATUS = -4        # OFDM_FRAME_HEADER


def live_and_unit(n_rows, quality=None, status=None):
    """(live bool [n_rows], u f32 [n_rows]).  Live: status 0 (or no status array), the quality row valid, its LLR unit finite and > 0;
    without quality rows every branch with status 0 is live and u = 1."""
    live = np.ones(n_rows, bool) if status is None else (np.asarray(status).reshape(n_rows) == 0)
    if quality is None:
        return live, np.ones(n_rows, np.float32)
    q = np.asarray(quality, np.float32).reshape(n_rows, QUALITY_FIELDS)
    u = q[:, Q_LLR_UNIT]
    with np.errstate(invalid="ignore"):
        live = live & (q[:, Q_VALID] == 1) & np.isfinite(u) & (u > 0)
    return live, u


def weights(n_frames, R, quality=None, status=None):
    """q int32 [n_frames * R]: rint(64 u_r / u_max) over the frame's live branches (f64 quotient, ties to even), 0 for a dead one"""
    assert 1 <= R <= MAX_BRANCHES
    live, u = live_and_unit(n_frames * R, quality, status)
    live, u = live.reshape(n_frames, R), u.reshape(n_frames, R).astype(np.float64)
    u_max = np.where(live, u, 0.0).max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        q = np.rint(64.0 * u / u_max)
    return np.where(live, q, 0.0).astype(np.int32).reshape(-1)


def counted(n_rows, n_llr, n_live=None):
    """n_r per branch row: its n_live entry clamped to [0, n_llr], n_llr without the array"""
    if n_live is None:
        return np.full(n_rows, n_llr, np.int64)
    return np.clip(np.asarray(n_live, np.int64).reshape(n_rows), 0, n_llr)


def combine(llr, R, quality=None, status=None, n_live=None):
    """llr int8 [n_frames * R, n_llr] -> (out int8 [n_frames, n_llr], q int32 [n_frames * R]):
    out[j] = clamp((sum over the branches counting at j of q_r L_r[j] + 32) >> 6, -127, 127), the shift arithmetic"""
    llr = np.asarray(llr, np.int8)
    rows, n_llr = llr.shape
    assert rows % R == 0
    n_frames = rows // R
    q = weights(n_frames, R, quality, status)
    n = counted(rows, n_llr, n_live)
    counts = np.arange(n_llr)[None, :] < n[:, None]
    prod = np.where(counts, llr.astype(np.int64) * q[:, None].astype(np.int64), 0)
    s = prod.reshape(n_frames, R, n_llr).sum(axis=1)
    return np.clip((s + 32) >> 6, -127, 127).astype(np.int8), q


def merge(R, status, nsym, quality=None):
    """The chain's per-frame verdict from its branches' status and live-symbol counts -> (status_f int32 [n_frames], nsym_f int32
    [n_frames]): status_f = 0 if a branch is live, else the first non-zero status in branch order, else (no branch live, every status 0)
    OFDM_FRAME_HEADER; nsym_f = the largest nsym over the live branches (0 without one)"""
    status = np.asarray(status, np.int32).reshape(-1, R)
    nsym = np.asarray(nsym, np.int32).reshape(-1, R)
    live, _ = live_and_unit(status.size, quality, status.reshape(-1))
    live = live.reshape(-1, R)
    st = np.zeros(status.shape[0], np.int32)
    for f in range(status.shape[0]):
        if not live[f].any():
            nz = status[f][status[f] != 0]
            st[f] = nz[0] if nz.size else HEADER_STATUS
    return st, np.where(live, nsym, 0).max(axis=1).astype(np.int32)
