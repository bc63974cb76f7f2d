"""The adaptive-supersampling contract of include/mbk.h ("Adaptive supersampling") in numpy: base and fine samples in, RGBA8 and
mask out.  Written from the header's text on top of render_model (colour, resolve): integers throughout."""
import numpy as np

import render_model as M

THRESHOLD_MAX = 256


def base_image(palette, inside, scale, offset, base_counts, base_nu):
    """B: the s = 1 render of the whole view, (H, W, 4) uint8."""
    return M.render_smooth(palette, inside, scale, offset, 1, base_counts, base_nu)


def refined_mask(base, threshold):
    """(H, W) bool from the base image of the WHOLE view: threshold 0 refines everything; otherwise a pixel is refined iff one
    of its up to eight neighbours inside the view differs from it by >= threshold in some channel, alpha included."""
    assert 0 <= threshold <= THRESHOLD_MAX
    b = np.asarray(base).astype(np.int64)
    h, w, _ = b.shape
    if threshold == 0:
        return np.ones((h, w), bool)
    mask = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            # pixels (y, x) whose neighbour (y + dy, x + dx) lies inside the view
            ys = slice(max(0, -dy), h - max(0, dy))
            xs = slice(max(0, -dx), w - max(0, dx))
            yn = slice(max(0, dy), h - max(0, -dy))
            xn = slice(max(0, dx), w - max(0, -dx))
            diff = np.abs(b[ys, xs] - b[yn, xn]).max(axis=2)
            mask[ys, xs] |= diff >= threshold
    return mask


def render_adaptive(palette, inside, scale, offset, s, threshold, base_counts, base_nu, fine_counts, fine_nu):
    """(rgba (H, W, 4) uint8, mask (H, W) uint8) of the whole view: a refined pixel is the render at s, any other the base."""
    base = base_image(palette, inside, scale, offset, base_counts, base_nu)
    mask = refined_mask(base, threshold)
    fine = M.render_smooth(palette, inside, scale, offset, s, fine_counts, fine_nu)
    assert fine.shape == base.shape
    return np.where(mask[..., None], fine, base), mask.astype(np.uint8)


def sample_stats(mask, mrd, s, base_counts, fine_counts, window=None):
    """(pixel_iterations, never_pixels) of a window (col0, row0, ncols, nrows; None: the view): the base samples of its pixels
    plus the s^2 fine samples of each refined one (at s = 1 a refined pixel's one sample IS its base sample: counted once).  A
    sample that never escapes costs mrd - 1 steps."""
    h, w = mask.shape
    c0, r0, nc, nr = (0, 0, w, h) if window is None else window
    cap = max(int(mrd) - 1, 0)

    def totals(counts):
        c = np.asarray(counts, np.int64)
        return int(np.where(c > 0, c, cap).sum()), int((c == 0).sum())

    m = np.asarray(mask, bool)[r0:r0 + nr, c0:c0 + nc]
    fine = np.asarray(fine_counts).reshape(h, s, w, s)[r0:r0 + nr, :, c0:c0 + nc, :]
    it_b, nv_b = totals(np.asarray(base_counts)[r0:r0 + nr, c0:c0 + nc])
    it_f, nv_f = totals(fine.transpose(0, 2, 1, 3)[m]) if s > 1 else (0, 0)
    return it_b + it_f, nv_b + nv_f


def halo(window, width, height):
    """The window (col0, row0, ncols, nrows) grown by one pixel on every side and clamped to the width x height view: the
    rectangle of the s = 1 image that decides which of the window's pixels are refined."""
    c0, r0, nc, nr = window
    hc0, hr0 = max(c0 - 1, 0), max(r0 - 1, 0)
    return hc0, hr0, min(c0 + nc + 1, width) - hc0, min(r0 + nr + 1, height) - hr0


def render_adaptive_window(palette, inside, scale, offset, s, threshold, window, width, height, halo_counts, halo_nu, fine_counts,
                           fine_nu):
    """render_adaptive for a window of a width x height view without the view: halo_counts / halo_nu are the base samples of
    halo(window, width, height), fine_counts / fine_nu the samples of the window at s (nrows * s by ncols * s).  A window pixel's
    neighbours all lie in the halo rectangle unless they lie outside the view, and the rule looks at no others: refined_mask on
    the halo rectangle, whose own border plays the view's where the view ends and is cut away where it does not, is the whole
    view's mask on the window."""
    c0, r0, nc, nr = window
    hc0, hr0, hnc, hnr = halo(window, width, height)
    assert np.asarray(halo_counts).shape == (hnr, hnc) and np.asarray(fine_counts).shape == (nr * s, nc * s)
    base = base_image(palette, inside, scale, offset, halo_counts, halo_nu)
    rows, cols = slice(r0 - hr0, r0 - hr0 + nr), slice(c0 - hc0, c0 - hc0 + nc)
    mask = refined_mask(base, threshold)[rows, cols]
    fine = M.render_smooth(palette, inside, scale, offset, s, fine_counts, fine_nu)
    return np.where(mask[..., None], fine, base[rows, cols]), mask.astype(np.uint8)
