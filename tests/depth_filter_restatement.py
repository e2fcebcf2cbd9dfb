"""The bilateral depth filter's contract (include/icp_hip.h) in numpy fp32: every operation in the contract's order,
one rounding each.  The tables are arguments -- `binding.depth_filter_tables` gives the ones the device uses, so nothing here evaluates exp
and the device's output can be asked for bit for bit.

  filter_depth(depth, radius, spatial, range_table, inv_bin)   the whole image at once, one tap of the window after the other
  filter_pixel(depth, u, v, radius, spatial, range_table, inv_bin)   the rule read out for one pixel, loop by loop (the cross-check)"""
import numpy as np

f32 = np.float32
MINF = f32(-np.inf)


def usable(d):
    """finite and > 0"""
    d = np.asarray(d, f32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def filter_depth(depth, radius, spatial, range_table, inv_bin):
    d = np.ascontiguousarray(depth, f32)
    r = int(radius)
    if r == 0:
        return d.copy()
    h, w = d.shape
    S = np.asarray(spatial, f32).reshape(2 * r + 1, 2 * r + 1); R = np.asarray(range_table, f32).reshape(256); ib = f32(inv_bin)
    pad = np.full((h + 2 * r, w + 2 * r), MINF, f32)          # outside the image: not usable, which is the rule's skip
    pad[r:r + h, r:r + w] = d
    okc = usable(d)
    num = np.zeros((h, w), f32); den = np.zeros((h, w), f32)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                n = pad[r + dy:r + dy + h, r + dx:r + dx + w]
                delta = n - d
                e = delta * delta
                t = e * ib
                ok = okc & usable(n) & (t < f32(256.0))
                q = np.where(ok, t, f32(0)).astype(np.int32)
                wgt = S[dy + r, dx + r] * R[q]
                num = np.where(ok, num + wgt * n, num)
                den = np.where(ok, den + wgt, den)
        return np.where(okc, num / den, d)


def filter_pixel(depth, u, v, radius, spatial, range_table, inv_bin):
    d = np.asarray(depth, f32); h, w = d.shape; r = int(radius)
    S = np.asarray(spatial, f32).reshape(-1); R = np.asarray(range_table, f32).reshape(256); ib = f32(inv_bin)
    c = d[v, u]
    if r == 0 or not usable(c):
        return c
    num = f32(0); den = f32(0)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                x, y = u + dx, v + dy
                if x < 0 or x >= w or y < 0 or y >= h:
                    continue
                n = d[y, x]
                if not usable(n):
                    continue
                delta = f32(n - c)
                e = f32(delta * delta)
                t = f32(e * ib)
                if not t < f32(256.0):
                    continue
                q = int(t)
                wgt = f32(S[(dy + r) * (2 * r + 1) + (dx + r)] * R[q])
                num = f32(num + f32(wgt * n))
                den = f32(den + wgt)
    return f32(num / den)


def window_bounds(depth, radius):
    """(min, max) of the usable depths in every pixel's window (NaN where the window has none)."""
    d = np.asarray(depth, f32); h, w = d.shape; r = int(radius)
    pad = np.full((h + 2 * r, w + 2 * r), np.nan, f32)
    pad[r:r + h, r:r + w] = np.where(usable(d), d, f32(np.nan))
    stack = np.stack([pad[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmin(stack, axis=0), np.nanmax(stack, axis=0)
