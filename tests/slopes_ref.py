"""The definition of gg_export_slopes (include/groundgrid_hip.h) in numpy, float32 throughout: what the kernels are held to on bits."""
import numpy as np

CHANNELS = ["grad_x", "grad_y", "tangent", "normal_z", "step", "min_confidence"]
FRESH = [np.float32(0.0), np.float32(0.0), np.float32(0.0), np.float32(1.0), np.float32(0.0), np.float32(1e-7)]


def slopes_reference(ground, groundpatch, res):
    """ground, groundpatch: (rows, cols) float32 arrays; res: np.float32.  Returns the six (rows, cols) float32 planes in GG_SLOPE_* order."""
    g = np.ascontiguousarray(ground, dtype=np.float32)
    w = np.ascontiguousarray(groundpatch, dtype=np.float32)
    assert g.ndim == 2 and g.shape == w.shape
    res = np.float32(res)
    rows, cols = g.shape
    r, c = np.arange(rows), np.arange(cols)
    r_lo, r_hi = np.maximum(r - 1, 0), np.minimum(r + 1, rows - 1)
    c_lo, c_hi = np.maximum(c - 1, 0), np.minimum(c + 1, cols - 1)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        gx = (g[r_lo, :] - g[r_hi, :]) / ((r_hi - r_lo).astype(np.float32) * res)[:, None]
        gy = (g[:, c_lo] - g[:, c_hi]) / ((c_hi - c_lo).astype(np.float32) * res)[None, :]
        s = gx * gx + gy * gy
        tangent = np.sqrt(s)
        normal_z = one / np.sqrt(s + one)
        step = np.zeros_like(g)
        conf = w.copy()
        # (a clamped index names a cell of the neighbourhood a second time: no maximum and no minimum changes by that)
        for rr in (r_lo, r, r_hi):
            for cc in (c_lo, c, c_hi):
                step = np.fmax(step, np.abs(g[np.ix_(rr, cc)] - g))
                conf = np.fmin(conf, w[np.ix_(rr, cc)])
    out = [gx, gy, tangent, normal_z, step, conf]
    assert all(p.dtype == np.float32 and p.shape == g.shape for p in out)
    return out
