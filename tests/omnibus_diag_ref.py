"""numpy restatement of the omnibus test for block-diagonal covariance structures (test infrastructure).

Vectorised over pixels, sequential over dates, with the rounding points of the generic-p oracle
(oracle/nd_oracle_impl.h:150-200) made explicit: `T` is the dtype of the planes, everything marked
`float64` is double.  Generic in the block structure so that it can be pinned:

  structure (2,)      one 2 x 2 block, planes [C11, C12re, C12im, C22]: the reference's own test
                      (nd/_change.pyx:46-77, 133-151, 224-257) -- must equal oracle.change_detection
  structure (1,) * q  q independent 1 x 1 blocks, planes [x_1 .. x_q]: the intensity-only test

For m equal blocks of size b:  det = product of the block determinants (left to right in T),
p = m b,  f = m b^2 (j - 1),  rho = rho(b, j, n),  omega2 = m omega2(b, j, n, rho)  (Box's expansion is
additive over independent blocks; for b = 1 this is f = q (j - 1), omega2 = -(q (j - 1) / 4)(1 - 1/rho)^2).

Planes are arrays with time on axis 0 and any pixel shape behind it.  Logarithms go through libm
(math.log), as in the oracle; numpy's vector log may differ from it in the last bit.
"""
import math

import numpy as np

from oracle import oracle as O


def _clog(x):
    """libm's log, element by element, on a float64 array (0 -> -inf, negative -> nan)."""
    x = np.asarray(x, np.float64)
    if x.size and bool(((x > 0.0) & (x < math.inf)).all()):
        return np.array(list(map(math.log, x.ravel().tolist())), np.float64).reshape(x.shape)
    out = np.empty(x.shape, np.float64)
    flat, oflat = x.ravel(), out.ravel()
    for i, v in enumerate(flat.tolist()):
        if v > 0.0:
            oflat[i] = math.log(v) if v != math.inf else math.inf
        elif v == 0.0:
            oflat[i] = -math.inf
        else:
            oflat[i] = math.nan
    return oflat.reshape(x.shape)


def _blocks(structure):
    structure = tuple(int(b) for b in structure)
    if not structure or any(b != structure[0] for b in structure) or structure[0] not in (1, 2):
        raise ValueError('structure must be m equal blocks of size 1 or 2, got %r' % (structure,))
    return structure[0], len(structure)


def _det(v, b):
    """product of the block determinants of one date (or of the sums), left to right in T"""
    if b == 2:
        dets = [(v[4 * i] * v[4 * i + 3]) - ((v[4 * i + 1] * v[4 * i + 1]) + (v[4 * i + 2] * v[4 * i + 2]))
                for i in range(len(v) // 4)]
    else:
        dets = list(v)
    d = dets[0]
    for e in dets[1:]:
        d = d * e
    return d


def constants(structure, j, n):
    """(f, rho, omega2) of the test over j dates, in double."""
    b, m = _blocks(structure)
    with np.errstate(all='ignore'):
        rho = O.rho(b, j, n) if j > 1 else math.nan
        omega2 = m * O.omega2(b, j, n, rho) if j > 1 else math.nan
    return float(m * b * b * (j - 1)), rho, omega2


def _prefix_log_q(planes, structure, n, l=0, last_only=False):
    """ln Q of every prefix ts[l : l + j], j = 1 .. k - l, as an array (k - l, pixels...) of float64
    (last_only: only the row of the whole of ts[l:] is filled in)."""
    b, m = _blocks(structure)
    T = planes[0].dtype.type
    k = planes[0].shape[0]
    shape = planes[0].shape[1:]
    prod = np.ones(shape, np.float64)
    sums = [np.zeros(shape, T) for _ in planes]
    out = np.empty((k - l,) + shape, np.float64)
    with np.errstate(all='ignore'):
        for i in range(l, k):
            v = [p[i] for p in planes]
            prod = prod * _det(v, b).astype(np.float64)
            sums = [s + x for s, x in zip(sums, v)]
            j = i - l + 1
            if last_only and i < k - 1:
                continue
            det_of_sum = _det(sums, b)
            pk = T(m * b) * T(j)
            out[i - l] = float(n) * (((float(pk) * math.log(float(j))) + _clog(prod))
                                     - (float(j) * _clog(det_of_sum.astype(np.float64))))
    return out


def log_q(planes, structure, n):
    """ln Q of the test over the whole series (float64, pixel shape)."""
    planes = [np.asarray(p) for p in planes]
    return _prefix_log_q(planes, structure, n, last_only=True)[-1]


def _z_of(logq, T, rho):
    with np.errstate(all='ignore'):
        return ((-2.0 * float(T(rho))) * logq).astype(T)


def _p_of(z, T, f, omega2):
    """P = T(P1 + omega2 T(T(P2) - T(P1))) of statistics z (array of T)."""
    zf = z.astype(np.float64).ravel().tolist()
    cdf = O.lib().oracle_cdf_chisq_P
    with np.errstate(all='ignore'):
        P1 = np.array([cdf(v, f) for v in zf], np.float64).astype(T)
        P2 = np.array([cdf(v, f + 4.0) for v in zf], np.float64).astype(T)
        d = (P2 - P1).astype(T)
        P = (P1.astype(np.float64) + (omega2 * d.astype(np.float64))).astype(T)
    return P.reshape(z.shape)


def single_test(planes, structure, n):
    """(z, P) of the test over the whole series, arrays of T with the pixel shape."""
    planes = [np.asarray(p) for p in planes]
    T = planes[0].dtype.type
    k = planes[0].shape[0]
    f, rho, omega2 = constants(structure, k, n)
    z = _z_of(log_q(planes, structure, n), T, rho)
    return z, _p_of(z, T, f, omega2)


class Series:
    """The tests of one stack, evaluated on demand and kept: change_detection at several thresholds
    shares them."""

    def __init__(self, planes, structure, n):
        self.planes = [np.asarray(p).reshape(np.asarray(p).shape[0], -1) for p in planes]
        self.shape = np.asarray(planes[0]).shape[1:]
        self.structure, self.n = tuple(structure), n
        self.T = self.planes[0].dtype.type
        self.k = self.planes[0].shape[0]
        self.npix = self.planes[0].shape[1]
        self._z, self._P, self._have = {}, {}, {}

    def z(self, l):
        """z of the tests over ts[l : l + j], row j - 1 (row 0, a single date, is not a test)."""
        if l not in self._z:
            logq = _prefix_log_q(self.planes, self.structure, self.n, l)
            z = np.empty(logq.shape, self.T)
            for j in range(1, self.k - l + 1):
                z[j - 1] = _z_of(logq[j - 1], self.T, constants(self.structure, j, self.n)[1])
            self._z[l] = z
        return self._z[l]

    def P(self, l, j, idx):
        """P of the test over ts[l : l + j] for the pixels idx."""
        key = (l, j)
        if key not in self._P:
            self._P[key] = np.zeros(self.npix, self.T)
            self._have[key] = np.zeros(self.npix, bool)
        need = idx[~self._have[key][idx]]
        if need.size:
            f, _, omega2 = constants(self.structure, j, self.n)
            self._P[key][need] = _p_of(self.z(l)[j - 1][need], self.T, f, omega2)
            self._have[key][need] = True
        return self._P[key][idx]


def change_detection(planes, structure, alpha, n, series=None):
    """The sequential search of nd/_change.pyx:224-257.  Returns (map uint8 (pixels..., k), z, P), z / P of
    the whole-series test.  `series`: a Series of the same stack, to share its tests between thresholds; its
    `closest` is set to the smallest |P - alpha| among the tests this search asked (NaN aside)."""
    S = series if series is not None else Series(planes, structure, n)
    closest = [math.inf]

    def asked(P):
        with np.errstate(all='ignore'):
            P = P.astype(np.float64)
            d = np.abs(P - alpha)
            if d.size and not np.isnan(d).all():
                closest[0] = min(closest[0], float(np.nanmin(d)))
            return P > alpha
    k, npix = S.k, S.npix
    change = np.zeros((npix, k), np.uint8)
    everyone = np.arange(npix)
    z0 = S.z(0)[k - 1].copy()
    P0 = S.P(0, k, everyone).copy()
    start = np.zeros(npix, np.int64)
    active = np.ones(npix, bool) if k >= 2 else np.zeros(npix, bool)
    while active.any():
        for l in np.unique(start[active]).tolist():
            idx = everyone[active & (start == l)]
            fires = asked(S.P(l, k - l, idx))                                # :241-242
            active[idx[~fires]] = False
            todo = idx[fires]
            for j in range(2, k - l + 1):                                    # :246-253
                if not todo.size:
                    break
                hit = asked(S.P(l, j, todo))
                found = todo[hit]
                change[found, l + j - 1] = 1
                start[found] = l + j - 1                                     # :255
                todo = todo[~hit]
            # (todo is empty here: the marginal test over k - l dates is the global test, which fired;
            #  r = (k - l) - 1 for the pixels whose only firing marginal is that one)
            assert not todo.size
        active &= start < k - 1                                              # :256
    S.closest = closest[0]
    return change.reshape(S.shape + (k,)), z0.reshape(S.shape), P0.reshape(S.shape)
