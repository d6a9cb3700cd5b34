"""The regions of a map restated on the host (include/nd_amd.h "Regions of a map").  With by_value=False the labels
ARE scipy.ndimage.label's: scipy numbers regions in raster order of their first pixel.  With by_value=True every
distinct foreground value is labelled by scipy on its own, the results are united and renumbered by first pixel in
raster order (tests/test_regions_cpu.py holds that to a flood fill).  Areas, sizes and the sieve follow from the
labels by np.bincount."""
import numpy as np
import scipy.ndimage as ndi


def structure(connectivity):
    assert connectivity in (4, 8)
    return ndi.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), bool)


def foreground(v, background=0):
    v = np.asarray(v)
    with np.errstate(invalid='ignore'):
        return (v != v.dtype.type(background)) & (v == v)


def label(v, connectivity=4, background=0, by_value=False):
    """one plane -> (labels int32, n)"""
    v = np.asarray(v)
    assert v.ndim == 2
    fg = foreground(v, background)
    if v.size == 0:
        return np.zeros(v.shape, np.int32), 0
    if not by_value:
        lab, n = ndi.label(fg, structure(connectivity), output=np.int32)
        return lab, int(n)
    united = np.zeros(v.shape, np.int64)
    n = 0
    # np.unique would merge nothing that == keeps apart, but it splits -0.0 from 0.0 nowhere either: go by ==
    todo = fg.copy()
    while todo.any():
        value = v[todo][0]
        same = fg & (v == value)
        lab, m = ndi.label(same, structure(connectivity), output=np.int32)
        united[same] = lab[same].astype(np.int64) + n
        n += int(m)
        todo &= ~same
    flat = united.ravel()
    idx = np.flatnonzero(flat)
    # a region's first pixel in raster order, and the regions ranked by it
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat[idx], idx)
    order = np.argsort(first[1:], kind='stable')
    rank = np.zeros(n + 1, np.int64)
    rank[1 + order] = 1 + np.arange(n)
    return rank[united].astype(np.int32), n


def sizes(labels, n):
    return np.bincount(labels.ravel(), minlength=n + 1)[1:].astype(np.int64)


def area(labels, n):
    s = np.concatenate(([0], sizes(labels, n)))
    return s[labels].astype(np.int32)


def sieve(v, min_size, connectivity=4, background=0, by_value=False, fill=None):
    v = np.asarray(v)
    lab, n = label(v, connectivity, background, by_value)
    out = v.copy()
    small = (lab > 0) & (area(lab, n) < min_size)
    out[small] = v.dtype.type(background if fill is None else fill)
    return out


def planes(fn, stack, *args, **kw):
    """fn over the planes of a (k, ny, nx) stack -> a list of its results"""
    return [fn(p, *args, **kw) for p in stack]
