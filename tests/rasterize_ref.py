"""The numpy restatement of the rasterize rule (include/nd_amd.h, README "Labels from polygons").

A polygon is a list of rings, a ring an (m, 2) array of pixel coordinates (px, py).  The centre of pixel (i, j) is
u = j + 0.5, v = i + 0.5.  For an edge let (x1, y1) be the endpoint with the smaller py and (x2, y2) the other:

    the edge crosses row i   iff  (y1 <= v) and not (y2 <= v)
    its abscissa             xc = x1 + ((v - y1) * (x2 - x1)) / (y2 - y1)        float64, this bracketing
    pixel (i, j) is inside   iff  the number of crossing edges of all rings with xc <= u is odd

Nothing here is shared with the package: tests/test_rasterize_cpu.py holds this file to matplotlib, to masks
enumerated by hand and to the tiling property; the GPU tests hold the kernels to this file, bit for bit.
"""
import numpy as np


def to_pixel(ring, transform):
    """(X, Y) -> (px, py) = ((X - c) / a, (Y - f) / e) for the transform (a, 0, c, 0, e, f)"""
    a, _, c, _, e, f = [float(t) for t in tuple(transform)[:6]]
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    return np.stack([(ring[:, 0] - c) / a, (ring[:, 1] - f) / e], axis=1)


def edges(rings):
    """x1, y1, x2, y2 of every edge of every ring with at least 3 vertices, (x1, y1) the endpoint of smaller py"""
    P, Q = [], []
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        if len(ring) < 3:
            continue
        P.append(ring)
        Q.append(np.roll(ring, -1, axis=0))
    if not P:
        z = np.zeros(0)
        return z, z, z, z
    P, Q = np.concatenate(P), np.concatenate(Q)
    swap = Q[:, 1] < P[:, 1]
    lo = np.where(swap[:, None], Q, P)
    hi = np.where(swap[:, None], P, Q)
    return lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1]


def polygon_mask(rings, ny, nx):
    """bool (ny, nx): the pixels whose centre the polygon holds"""
    x1, y1, x2, y2 = edges(rings)
    mask = np.zeros((ny, nx), bool)
    u = np.arange(nx) + 0.5
    for i in range(ny):
        v = i + 0.5
        cross = (y1 <= v) & ~(y2 <= v)
        if not cross.any():
            continue
        a1, b1, a2, b2 = x1[cross], y1[cross], x2[cross], y2[cross]
        xc = a1 + ((v - b1) * (a2 - a1)) / (b2 - b1)
        mask[i] = ((xc[:, None] <= u[None, :]).sum(0) & 1).astype(bool)
    return mask


def burn(polys, values, ny, nx, layer=None, nlayers=1, fill=0, dtype=None):
    """(nlayers, ny, nx): every polygon in turn replaces what lies under it in its layer, so the highest index
    wins.  dtype: that of `values` (integers int64, floats float64) unless given."""
    values = np.asarray(values)
    if dtype is None:
        dtype = np.float64 if values.dtype.kind == 'f' else np.int64
    out = np.full((nlayers, ny, nx), fill, dtype=dtype)
    for p, rings in enumerate(polys):
        l = 0 if layer is None else int(layer[p])
        out[l][polygon_mask(rings, ny, nx)] = values[p]
    return out


def pack(polys):
    """-> verts (nverts, 2) float64, ring_offsets, poly_offsets (int64) of a list of ring lists"""
    verts, ring_offsets, poly_offsets = [], [0], [0]
    for rings in polys:
        for ring in rings:
            ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
            verts.append(ring)
            ring_offsets.append(ring_offsets[-1] + len(ring))
        poly_offsets.append(len(ring_offsets) - 1)
    verts = np.concatenate(verts) if verts else np.zeros((0, 2))
    return verts, np.asarray(ring_offsets, np.int64), np.asarray(poly_offsets, np.int64)


def distance_to_edges(rings, ny, nx):
    """(ny, nx) distance in pixels from every centre to the nearest edge of any ring (inf without edges)"""
    uu, vv = np.meshgrid(np.arange(nx) + 0.5, np.arange(ny) + 0.5)
    best = np.full((ny, nx), np.inf)
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        if len(ring) < 2:
            continue
        nxt = np.roll(ring, -1, axis=0)
        for (ax, ay), (bx, by) in zip(ring, nxt):
            dx, dy = bx - ax, by - ay
            L2 = dx * dx + dy * dy
            t = np.zeros_like(uu) if L2 == 0 else np.clip(((uu - ax) * dx + (vv - ay) * dy) / L2, 0, 1)
            best = np.minimum(best, np.hypot(uu - (ax + t * dx), vv - (ay + t * dy)))
    return best
