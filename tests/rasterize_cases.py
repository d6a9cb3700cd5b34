"""The polygons the rasterize tests share (tests/test_rasterize_cpu.py, tests/test_rasterize_gpu.py,
tools/fuzz_parity.py).  Everything is in pixel coordinates (px, py) unless a transform is named."""
import numpy as np

MAX_CROSSINGS = 256         # ND_AMD_RASTERIZE_MAX_CROSSINGS; the GPU test checks the mirror in kernels


def star(rng, cx, cy, r, m, spread=0.6):
    """a star-shaped ring of m vertices around (cx, cy): sorted random angles, radii in [(1 - spread) r, r]"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    rad = r * rng.uniform(1 - spread, 1, m)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def snap(ring):
    """vertices on the half-integer grid, where pixel centres and the lines through them lie"""
    return np.round(ring * 2) / 2


def random_polygon(rng, ny, nx, hole=False, snapped=False, m=None):
    """one star polygon that may stick out of the raster, with a star hole inside its inner radius"""
    m = int(rng.integers(3, 41)) if m is None else m
    cx, cy = rng.uniform(0, nx), rng.uniform(0, ny)
    r = rng.uniform(0.3, 0.7) * max(nx, ny)
    rings = [star(rng, cx, cy, r, m)]
    if hole:
        rings.append(star(rng, cx, cy, 0.35 * r, int(rng.integers(3, 12)), spread=0.3)[::-1])
    return [snap(g) for g in rings] if snapped else rings


def matplotlib_cases():
    """the 40 cases of the comparison with matplotlib: (name, rings, ny, nx); 3 to 40 vertices, rasters of 5 to 70
    pixels a side, every second with a hole, every fifth snapped to half-integers"""
    out = []
    for k in range(40):
        rng = np.random.default_rng([20261019, k])
        ny, nx = int(rng.integers(5, 71)), int(rng.integers(5, 71))
        out.append(('star%02d' % k, random_polygon(rng, ny, nx, hole=k % 2 == 1, snapped=k % 5 == 0), ny, nx))
    return out


def snapped_cases():
    return [c for k, c in enumerate(matplotlib_cases()) if k % 5 == 0]


def regular_ring(m, cx, cy, r, phase=0.1):
    ang = phase + 2 * np.pi * np.arange(m) / m
    return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)


def comb(crossings, x0=0.31, x1=39.7, ybase=0.2, ytop=7.6, width=0.05):
    """a comb whose teeth are `width` pixel wide, on a spine below the first centre line: every row of an 8-row
    raster has `crossings` crossings, two per tooth"""
    teeth = crossings // 2
    assert crossings == 2 * teeth and teeth >= 1
    pitch = (x1 - x0) / teeth
    assert pitch > width
    spine = ybase + 0.2
    pts = [(x0, ybase), (x1, ybase), (x1, spine)]
    for t in range(teeth - 1, -1, -1):
        left = x0 + t * pitch
        pts += [(left + width, spine), (left + width, ytop), (left, ytop), (left, spine)]
    return [np.asarray(pts, dtype=np.float64)]


def fan(rng, ny, nx, m=9):
    """a random convex polygon and the fan of triangles around an interior point: (polygon rings, [triangle rings])
    -- the shared edges are diagonals, the triangles tile the polygon"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    hull = np.stack([nx / 2 + 0.45 * nx * np.cos(ang), ny / 2 + 0.45 * ny * np.sin(ang)], axis=1)
    w = rng.dirichlet(np.ones(m))
    centre = (w[:, None] * hull).sum(0)
    tris = [[np.stack([centre, hull[k], hull[(k + 1) % m]])] for k in range(m)]
    return [hull], tris


def overlapping(rng, n, ny, nx):
    """n polygons all over (and partly off) the raster, some with holes, every seventh snapped"""
    polys = []
    for k in range(n):
        g = random_polygon(rng, ny, nx, hole=k % 3 == 0, m=int(rng.integers(3, 13)))
        scale = rng.uniform(0.15, 0.6)
        c = g[0].mean(0)
        g = [c + (ring - c) * scale for ring in g]
        polys.append([snap(ring) for ring in g] if k % 7 == 0 else g)
    return polys


def parcels(rng, n, ny, nx, mmin=4, mmax=12):
    """n small random parcels (one ring each) scattered over the raster: the benchmark's first workload"""
    polys = []
    r = 0.5 * np.sqrt(ny * nx / max(n, 1)) * 1.5
    for _ in range(n):
        polys.append([star(rng, rng.uniform(0, nx), rng.uniform(0, ny), r, int(rng.integers(mmin, mmax + 1)))])
    return polys
