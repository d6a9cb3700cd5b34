"""kernels.label_regions / region_sizes / sieve_regions and nd_amd.regions on the GPU against scipy.ndimage.label and
the by_value restatement (tests/regions_ref.py): equal everywhere, no tolerance.  The shapes are the smallest at which
a tiled union-find (tiles of 32 x 64) can go wrong."""
import numpy as np
import pytest

from tests import regions_cases as cases
from tests import regions_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_masks_equal_scipy(K, shape, connectivity):
    import scipy.ndimage as ndi
    rng = np.random.default_rng([11, shape[0], shape[1], connectivity])
    stack = np.stack([cases.mask(rng, shape, d) for d in cases.DENSITIES])
    lab, counts, _ = cases.device_label(K, stack, connectivity)
    for p, plane in enumerate(stack):
        want, n = ndi.label(plane != 0, ref.structure(connectivity), output=np.int32)
        assert counts[p] == n
        cases.assert_same(lab[p], want)


@pytest.mark.parametrize('name', sorted(cases.adversarial()))
def test_adversarial_planes(K, name):
    plane = cases.adversarial()[name]
    for connectivity in (4, 8):
        lab, counts = cases.check_label(K, plane[None], connectivity, area=True)
        if name == 'serpentine' and connectivity == 4:
            assert counts[0] == 1 and lab[0, -1, -1] == 1
        if name == 'checkerboard':
            assert counts[0] == (5250 if connectivity == 4 else 1)


@pytest.mark.parametrize('dtype', ['uint8', 'int32', 'int64', 'float32', 'float64'])
def test_by_value(K, dtype):
    rng = np.random.default_rng([12, len(dtype), ord(dtype[0])])
    stack = np.stack([cases.class_map(rng, (65, 129), nclass, dtype) for nclass in (2, 3, 5)])
    for connectivity in (4, 8):
        lab, counts = cases.check_label(K, stack, connectivity, 0, True, area=True)
        cases.check_label(K, stack, connectivity, 3, True)
        # classes that touch are kept apart: more regions than without by_value
        assert (counts >= cases.want_label(stack, connectivity, 0, False)[1]).all()
    cases.check_sieve(K, stack, 5, 4, 3, True, fill=None)
    cases.check_sieve(K, stack, 5, 8, 0, True, fill=4)


def test_int64_last_bit_and_negative_zero(K):
    a, b = 2 ** 53, 2 ** 53 + 1
    v = np.array([[[a, b, b, 0, a]]], np.int64)
    lab, counts = cases.check_label(K, v, 4, 0, True)
    assert counts[0] == 3 and list(lab[0, 0]) == [1, 2, 2, 0, 3]
    lab, counts = cases.check_label(K, v, 4, a, False)
    assert list(lab[0, 0]) == [0, 1, 1, 1, 0]
    f = np.array([[[-0.0, 0.0, 1.0, np.nan, 1.0]]], np.float32)
    lab, counts = cases.check_label(K, f, 8, 7, True)
    assert list(lab[0, 0]) == [1, 1, 2, 0, 3]
    lab, counts = cases.check_label(K, f, 8, 0, False)
    assert list(lab[0, 0]) == [0, 0, 1, 0, 2]
    got = cases.check_sieve(K, f, 2, 4, 7, True, fill=5)
    assert np.signbit(got[0, 0, 0]) and np.isnan(got[0, 0, 3]) and list(got[0, 0, [2, 4]]) == [5, 5]


@pytest.mark.parametrize('layout', cases.LAYOUTS)
@pytest.mark.parametrize('strided', [False, True], ids=['packed', 'strided'])
def test_batches_layouts_and_strided_outputs(K, layout, strided):
    rng = np.random.default_rng([13, len(layout), strided])
    stack = np.stack([cases.mask(rng, (70, 133), d, 'bool') for d in (0.59, 0.41, 0.0, 1.0, 0.59)])
    lab, counts = cases.check_label(K, stack, 4, area=True, layout=layout, strided=strided)
    assert counts[2] == 0 and counts[3] == 1
    # labels restart per plane
    assert all(lab[p].max() == counts[p] for p in range(5))
    cases.check_sieve(K, stack, 4, 8, layout=layout, strided=strided)
    sizes = cases.device_sizes(K, stack, 8, layout=layout)
    wl, wc = cases.want_label(stack, 8)
    for s, l, n in zip(sizes, wl, wc):
        assert np.array_equal(s, ref.sizes(l, n))


def test_two_dimensional_and_four_dimensional_inputs(K, device):
    import torch
    rng = np.random.default_rng(14)
    m = cases.mask(rng, (2, 3, 40, 70), 0.5)
    labels, counts = K.label_regions(torch.from_numpy(m).to(device), 8, dims=('a', 'time', 'y', 'x'))
    assert counts.shape == (2, 3) and labels.shape == m.shape
    wl, wc = cases.want_label(m.reshape(6, 40, 70), 8)
    cases.assert_same(labels.cpu().numpy().reshape(6, 40, 70), wl)
    assert np.array_equal(counts.cpu().numpy().reshape(-1), wc)
    sizes, offsets = K.region_sizes(labels, counts, dims=('a', 'time', 'y', 'x'))
    assert np.array_equal(sizes.cpu().numpy(), np.concatenate([ref.sizes(l, n) for l, n in zip(wl, wc)]))
    assert np.array_equal(offsets, np.concatenate(([0], np.cumsum(wc))))
    lab2, cnt2 = K.label_regions(torch.from_numpy(m[0, 0]).to(device), 8)
    assert cnt2.shape == () and int(cnt2) == wc[0]
    cases.assert_same(lab2.cpu().numpy(), wl[0])


def test_workspace_cap_walks_the_batch_in_chunks(K, monkeypatch):
    rng = np.random.default_rng(15)
    stack = np.stack([cases.mask(rng, (50, 70), 0.55) for _ in range(5)])
    monkeypatch.setattr(K, 'REGIONS_WORKSPACE_CAP', 2 * (50 * 70 * 8 + 600))        # two planes per call
    assert K._region_chunks(5, 50, 70, True) == [(0, 2), (2, 4), (4, 5)]
    cases.check_label(K, stack, 4, area=True)
    cases.check_sieve(K, stack, 3, 4)


@pytest.mark.parametrize('min_size', [0, 1, 2, 5, 10 ** 6])
def test_sieve(K, min_size):
    rng = np.random.default_rng([16, min_size])
    stack = np.stack([cases.mask(rng, (65, 129), d) for d in (0.3, 0.59)]) * 3
    for connectivity in (4, 8):
        got = cases.check_sieve(K, stack, min_size, connectivity)
        cases.check_sieve(K, stack, min_size, connectivity, fill=7)
        if min_size <= 1:
            cases.assert_same(got, stack)
        if min_size == 10 ** 6:
            assert not got.any()


def test_repeatable(K):
    rng = np.random.default_rng(17)
    for plane in (cases.serpentine(), cases.mask(rng, (131, 257), 0.59)):
        first = cases.device_label(K, plane[None], 4, area=True)
        second = cases.device_label(K, plane[None], 4, area=True)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        assert (cases.device_sieve(K, plane[None], 4).tobytes() == cases.device_sieve(K, plane[None], 4).tobytes())


def test_errors(K, device):
    import torch
    t = torch.zeros((4, 5), dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match='connectivity'):
        K.label_regions(t, connectivity=6)
    with pytest.raises(ValueError, match='representable'):
        K.label_regions(t, background=256)
    with pytest.raises(ValueError, match='representable'):
        K.sieve_regions(t, 3, fill=-1)
    with pytest.raises(TypeError):
        K.label_regions(t.to(torch.int16))
    with pytest.raises(TypeError, match='complex'):
        K.sieve_regions(t.to(torch.complex64), 3)
    with pytest.raises(ValueError, match='overlap'):
        K.sieve_regions(t, 3, out=t)
    with pytest.raises(ValueError, match='labels must be'):
        K.label_regions(t, labels=torch.zeros((4, 5), dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match='dims'):
        K.label_regions(t, dims=('time', 'x'))
    # empty inputs are served
    labels, counts = K.label_regions(torch.zeros((3, 0, 5), dtype=torch.uint8, device=device))
    assert labels.shape == (3, 0, 5) and counts.tolist() == [0, 0, 0]
    assert K.sieve_regions(torch.zeros((0, 4, 5), dtype=torch.uint8, device=device), 3).shape == (0, 4, 5)


# ---- the container layer -----------------------------------------------------------------------------------------
def test_omnibus_change_map_sieved_end_to_end(device):
    import torch
    from nd_amd import synth, xr_lite
    from nd_amd.change import OmnibusTest
    from nd_amd.regions import Sieve, label_regions, region_sizes, sieve
    k, ny, nx = 6, 70, 90
    stack = synth.wishart_c2_stack(k, ny, nx, looks=9, seed=21, device=device, change_frac=0.05)
    coords = {'time': np.arange(k), 'y': 10.0 - np.arange(ny), 'x': 5.0 + np.arange(nx)}
    ds = xr_lite.Dataset(coords=coords, attrs={'crs': 'none'})
    for name, plane in zip(('C11', 'C12__re', 'C12__im', 'C22'), stack):
        ds[name] = (('time', 'y', 'x'), plane)
    change = OmnibusTest(n=9, alpha=0.01).apply(ds)
    sieved = Sieve(min_size=4).apply(change)
    assert tuple(sieved.dims) == tuple(change.dims) and sieved.name == change.name
    assert sieved.attrs == change.attrs
    for c in coords:
        assert np.array_equal(np.asarray(sieved.coords[c]), coords[c])
    assert torch.is_tensor(sieved.values) and sieved.values.dtype == torch.bool
    assert sieved.values.stride() == change.values.stride()
    at = tuple(change.dims).index('time')
    got = np.moveaxis(sieved.values.cpu().numpy(), at, 0)
    host = np.moveaxis(change.values.cpu().numpy(), at, 0)
    assert 0 < host.mean() < 1
    for t in range(k):
        cases.assert_same(np.ascontiguousarray(got[t]), ref.sieve(host[t], 4))
    assert sieve(change, 4).equals(sieved)
    # the same map with the detections as background: the small no-change specks are filled, and there are some
    filled = np.moveaxis(Sieve(4, background=True).apply(change).values.cpu().numpy(), at, 0)
    for t in range(k):
        cases.assert_same(np.ascontiguousarray(filled[t]), ref.sieve(host[t], 4, background=True))
    assert filled.sum() > host.sum()

    # numpy in, numpy out; attrs['n_regions'] per plane in plane order
    host_da = xr_lite.DataArray(np.ascontiguousarray(change.values.cpu().numpy()), change.dims, change.coords,
                                {'a': 1}, 'change')
    lab = label_regions(host_da, connectivity=8)
    assert isinstance(lab.values, np.ndarray) and lab.values.dtype == np.int32 and lab.attrs['a'] == 1
    wl, wc = cases.want_label(host, 8)
    assert lab.attrs['n_regions'] == [int(n) for n in wc] and all(type(n) is int for n in lab.attrs['n_regions'])
    cases.assert_same(np.ascontiguousarray(np.moveaxis(lab.values, at, 0)), wl)
    sizes = region_sizes(host_da, connectivity=8)
    assert len(sizes) == k and all(np.array_equal(s, ref.sizes(l, n)) for s, l, n in zip(sizes, wl, wc))
    out = Sieve(3, connectivity=8).apply(host_da)
    assert isinstance(out.values, np.ndarray) and out.values.dtype == np.bool_

    # a Dataset: variables with y and x are processed, the others pass through
    both = xr_lite.Dataset(coords=coords)
    both['change'] = (tuple(change.dims), change.values)
    both['classes'] = (('y', 'x'), torch.from_numpy(cases.class_map(np.random.default_rng(5), (ny, nx), 4, 'int32'))
                       .to(device))
    both['dates'] = (('time',), np.arange(k))
    res = Sieve(4, by_value=True, fill=1).apply(both)
    assert list(res.data_vars) == ['change', 'classes', 'dates'] and res['dates'].values is both['dates'].values
    cases.assert_same(res['classes'].values.cpu().numpy(),
                      ref.sieve(both['classes'].values.cpu().numpy(), 4, 4, 0, True, 1))
    with pytest.raises(ValueError, match='connectivity'):
        label_regions(change, connectivity=5)
    cplx = xr_lite.DataArray(torch.zeros((4, 5), dtype=torch.complex64, device=device), ('y', 'x'))
    with pytest.raises(TypeError, match='complex'):
        Sieve(3).apply(cplx)
