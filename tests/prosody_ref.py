"""NumPy restatement of the prosody controls (include/vits_prosody.h): float32 where the device is float32, float64 for the fit.

Item b, token t < lengths[b].  ls_b = item_scales[b, 1] when item_scales is given, else length_scale.
  free-running  w_t = fp32(exp(logw_t)) * ls_b, then * token_length_scale[b, t] when given; d0_t = max(int(ceil(w_t)), 0); u_t = float64(w_t)
  forced        d0_t = max(forced[b, t], 0); u_t = float64(d0_t)
  no fit        d_t = d0_t + pause_t
  fit F_b > 0   U = sum u, P = sum pause, s = (F_b - P) / U; c_t = rint(s * sum_{j<=t} u_j) (float64, half-even), c_{-1} = 0;
                d_t = c_t - c_{t-1} + pause_t; the item has exactly F_b frames; fit_ratio = s (1 without a fit)
                refused: F_b <= P, U == 0, s outside [0.25, 4]
cum is the inclusive cumulative sum over the item's own tokens (constant beyond them), y_length = max(sum d, 1)."""
import numpy as np

MAX_TOKEN_SCALE = 16.0
FIT_RATIO = (0.25, 4.0)


class FitRefused(ValueError):
    pass


def base(logw, forced, lengths, length_scale=1.0, item_scales=None, token_length_scale=None):
    """-> (d0 int64 [B, T], u float64 [B, T], w float32 [B, T] or None), zero at and beyond lengths[b]"""
    src = forced if forced is not None else logw
    B, T = np.asarray(src).shape
    lengths = np.asarray(lengths, np.int64)
    mask = np.arange(T)[None, :] < lengths[:, None]
    if forced is not None:
        if token_length_scale is not None:
            raise ValueError("token_length_scale with forced durations")
        d0 = np.where(mask, np.maximum(np.asarray(forced, np.int64), 0), 0)
        return d0, d0.astype(np.float64), None
    ls = np.full((B, 1), length_scale, np.float32) if item_scales is None else np.asarray(item_scales, np.float32)[:, 1:2]
    w = np.exp(np.asarray(logw, np.float32)).astype(np.float32) * ls
    if token_length_scale is not None:
        w = w * np.asarray(token_length_scale, np.float32)
    w = np.where(mask, w.astype(np.float32), np.float32(0))
    d0 = np.where(mask, np.maximum(np.ceil(w).astype(np.int64), 0), 0)
    return d0, w.astype(np.float64), w


def regulate(logw, forced, lengths, length_scale=1.0, item_scales=None, token_length_scale=None, token_pause=None, fit_frames=None):
    """-> (durations int32 [B, T], cum int32 [B, T], y_lengths int64 [B], fit_ratio float64 [B])"""
    d0, u, _ = base(logw, forced, lengths, length_scale, item_scales, token_length_scale)
    B, T = d0.shape
    lengths = np.asarray(lengths, np.int64)
    mask = np.arange(T)[None, :] < lengths[:, None]
    pause = np.zeros((B, T), np.int64) if token_pause is None else np.where(mask, np.asarray(token_pause, np.int64), 0)
    d = d0 + pause
    ratio = np.ones(B, np.float64)
    for b in range(B):
        F = 0 if fit_frames is None else int(np.asarray(fit_frames)[b])
        if F <= 0:
            continue
        U, P = float(u[b].sum()), int(pause[b].sum())
        if F <= P or U == 0.0:
            raise FitRefused(f"item {b}: F = {F}, P = {P}, U = {U}")
        s = (float(F) - float(P)) / U
        if not FIT_RATIO[0] <= s <= FIT_RATIO[1]:
            raise FitRefused(f"item {b}: F = {F}, P = {P}, s = {s}")
        c = np.rint(s * np.cumsum(u[b])).astype(np.int64)  # (np.rint rounds half to even)
        d[b] = np.diff(c, prepend=0) + pause[b]
        ratio[b] = s
    cum = np.cumsum(d, axis=1)
    ylen = np.maximum(cum[:, -1], 1)
    return d.astype(np.int32), cum.astype(np.int32), ylen.astype(np.int64), ratio


def fit_margin(logw, forced, lengths, fit_frames, length_scale=1.0, item_scales=None, token_length_scale=None, token_pause=None):
    """min over the fitted items and their tokens of |frac(s * prefix_t) - 0.5|: how far every rounding of the fit is from a tie"""
    d0, u, _ = base(logw, forced, lengths, length_scale, item_scales, token_length_scale)
    _, _, _, ratio = regulate(logw, forced, lengths, length_scale, item_scales, token_length_scale, token_pause, fit_frames)
    m = 0.5
    for b in range(d0.shape[0]):
        L = int(np.asarray(lengths)[b])
        if int(np.asarray(fit_frames)[b]) <= 0 or L == 0:
            continue
        x = ratio[b] * np.cumsum(u[b, :L])
        m = min(m, float(np.abs((x - np.floor(x)) - 0.5).min()))
    return m


def ceil_margin(w, lengths=None):
    """min_t |w - rint(w)| / w in float64 over the valid tokens (w > 0): how far every ceil is from flipping under an ulp of expf"""
    w = np.asarray(w, np.float64)
    if lengths is not None:
        w = w[np.arange(w.shape[-1])[None, :] < np.asarray(lengths, np.int64)[:, None]]
    w = w[w > 0]
    return float((np.abs(w - np.rint(w)) / w).min()) if w.size else 0.5
