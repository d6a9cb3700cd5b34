"""Regenerate tests/golden/coreg_skimage.npz: Coregistration (nd/warp.py:1104-1163) as scikit-image 0.18
computes it, recorded on small stacks.  Needs scikit-image 0.18 (with its numpy / scipy); imports
nothing else:

    python tests/golden/make_coreg_golden.py

Cases (planar (time, y, x) inputs, quantised to multiples of 2^-8 so that float32 and float64 hold
the same values and the file compresses):
  f32_u10  float32, 4 variables x 6 dates x 30 x 38, upsampling 10, reference 2, one NaN in C22
  f64_u50  float64, 3 variables x 5 dates x 30 x 38, upsampling 50, reference 3
  f32_u1   float32, 3 variables x 5 dates x 24 x 32, upsampling 1, reference 4
(sizes kept small: the recorded outputs do not compress)
Every case records the inputs, skimage's shifts (k x 2, 0 at the reference) and its outputs.
C11 / C22 are positive (0 lies outside their range: the cval-preserve rule applies), C12 is signed.

ref50: the set-up of the reference's own test (nd/tests/test_coregister.py:9-30, 200 x 200 x 50
float64, Coregistration(upsampling=50)): skimage's 50 shifts and its outputs at a fixed sample of
(y, x, time) positions per variable, plus the shifts the set-up introduced.
"""
import os
import warnings

import numpy as np
import scipy.ndimage as ndi
import skimage
import skimage.registration
import skimage.transform

HERE = os.path.dirname(os.path.abspath(__file__))
VARS = ('C11', 'C12__re', 'C12__im', 'C22')


def coregister(planes, reference, u):
    """planes {name: (k, ny, nx)} -> ({name: out}, shifts): the reference's _coregister loop."""
    k = planes['C11'].shape[0]
    out = {n: a.copy() for n, a in planes.items()}
    sh = np.zeros((k, 2))
    for t in range(k):
        if t == reference:
            continue
        s = skimage.registration.phase_cross_correlation(planes['C11'][t], planes['C11'][reference],
                                                         upsample_factor=u)[0]
        sh[t] = s
        tf = skimage.transform.AffineTransform(translation=(s[1], s[0]))
        for n, a in planes.items():
            out[n][t] = skimage.transform.warp(a[t], tf, order=3)
    return out, sh


def stack(seed, k, ny, nx, nvars, dtype):
    rng = np.random.RandomState(seed)
    base = ndi.gaussian_filter(rng.normal(size=(ny + 16, nx + 16)), 2.5)
    base = (base - base.min()) / (base.max() - base.min())
    planes = {}
    for v in VARS[:nvars]:
        p = np.empty((k, ny, nx))
        for t in range(k):
            dy, dx = rng.uniform(-3, 3, 2)
            moved = ndi.shift(base, (dy, dx), order=3, mode='nearest')[8:8 + ny, 8:8 + nx]
            noise = rng.normal(scale=0.05, size=(ny, nx))
            p[t] = 0.2 + 3.0 * moved + noise if v in ('C11', 'C22') else 2.0 * moved - 1.0 + noise
        planes[v] = (np.round(p * 256) / 256).astype(dtype)
    if 'C11' in planes:
        planes['C11'] = np.abs(planes['C11']) + np.asarray(1 / 256, dtype)
    return planes


def reference_setup():
    """nd/tests/test_coregister.py:create_misaligned_dataset(dims={'y': 200, 'x': 200, 'time': 50})."""
    np.random.seed(0)
    np.random.seed(42)                       # generate_test_dataset re-seeds
    names = ('C11', 'C12__im', 'C12__re', 'C22')
    data = {n: np.random.normal(0, 1, (200, 200, 50)) for n in names}
    shifts = np.random.rand(50, 2)
    shifts[0, :] = 0
    for n in names:
        d0 = ndi.gaussian_filter(data[n][:, :, 0], 3)
        d0 = d0 / d0.max()
        a = data[n] / data[n].max() + d0[:, :, None]
        for t in range(1, 50):
            tf = skimage.transform.AffineTransform(translation=shifts[t, :])
            a[:, :, t] = skimage.transform.warp(a[:, :, t], tf, order=3)
        data[n] = a
    return data, shifts


def main():
    assert skimage.__version__.startswith('0.18'), skimage.__version__
    warnings.filterwarnings('ignore')
    rec = {}
    cases = [('f32_u10', 1, 6, 30, 38, 4, np.float32, 10, 2), ('f64_u50', 2, 5, 30, 38, 3, np.float64, 50, 3),
             ('f32_u1', 3, 5, 24, 32, 3, np.float32, 1, 4)]
    for name, seed, k, ny, nx, nvars, dtype, u, ref in cases:
        planes = stack(seed, k, ny, nx, nvars, dtype)
        if name == 'f32_u10':
            planes['C22'][3, 17, 23] = np.nan          # a NaN outside C11: that plane turns NaN
        out, sh = coregister(planes, ref, u)
        rec[name + '/meta'] = np.array([u, ref])
        rec[name + '/shifts'] = sh
        for v in planes:
            rec[name + '/in/' + v] = planes[v]
            rec[name + '/out/' + v] = out[v]
    data, introduced = reference_setup()
    planes = {n: np.ascontiguousarray(np.moveaxis(a, -1, 0)) for n, a in data.items()}
    out, sh = coregister(planes, 0, 50)
    rng = np.random.RandomState(7)
    idx = np.stack([rng.randint(0, 50, 1000), rng.randint(0, 200, 1000), rng.randint(0, 200, 1000)], 1)
    rec['ref50/shifts'] = sh
    rec['ref50/introduced'] = introduced
    rec['ref50/sample_tyx'] = idx.astype(np.int16)
    for n in planes:
        rec['ref50/sample/' + n] = out[n][idx[:, 0], idx[:, 1], idx[:, 2]]
    np.savez_compressed(os.path.join(HERE, 'coreg_skimage.npz'), **rec)


if __name__ == '__main__':
    main()
