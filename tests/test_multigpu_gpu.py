"""Multi-rank checks of the tile layer with the REAL HIP kernels.

  * `test_shared_gpu_...`: three fresh processes that SHARE the one GPU of a development / driver
    box, torch.distributed over `gloo` (RCCL refuses two ranks on one device; the halo pieces of
    the device shards are staged through the host, nd_amd/tiles.py): the same worker as the RCCL
    test below, so the sharded kernels, the in-place margin exchange on device buffers and the
    global-edge reflection run across ranks on every box;

  * `test_bench_launch_line_with_two_ranks`: the driver's N > 1 launch line of bench.py with two
    ranks sharing the GPU over gloo (ND_AMD_BENCH_REHEARSE) -- the sharding, reduction and
    one-JSON-line logic of the scaling bench, which only the driver can run on real 8-GPU nodes.

Two-GPU checks (skipped on a one-GPU box):

  * torch.distributed over `nccl`, one fresh process per GPU: halo exchange into the shard margins,
    then boxcar_rows / nlmeans_rows / nlmeans_then_omnibus on tile+halo, against the unsharded
    result computed by rank 0 on its own GPU -- bit for bit
    (nd/tests/test_filters_common.py:54-60: njobs=2 == serial, with the real filter);
  * one process driving two devices: `Filter.apply(ds, devices=[0, 1])` and
    `OmnibusTest(devices=[0, 1])` == the single-device result (the multi-worker hook of
    nd/algorithm.py:57-68).
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ngpu():
    import torch
    return torch.cuda.device_count()          # does not initialise the GPU on this image


needs2 = pytest.mark.skipif(_ngpu() < 2, reason='needs at least two GPUs')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, ret, backend='nccl', shared_gpu=False):
    import torch
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    idx = 0 if shared_gpu else rank
    torch.cuda.set_device(idx)
    dev = torch.device('cuda', idx)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from nd_amd import kernels, tiles
        k, ny, nx = 6, 301, 517                       # odd sizes: unequal blocks, ragged tiles
        g = torch.Generator().manual_seed(12)
        full = (torch.rand((4, k, ny, nx), generator=g) + 0.25)
        full[1] -= 0.75
        full[2] -= 0.75
        full[1] *= 0.3
        full[2] *= 0.3
        full[0, k // 2:, 100:200, 150:400] *= 6.0     # a step the omnibus test must find
        full[3, k // 2:, 100:200, 150:400] *= 6.0
        r, f = (1, 3, 3), (1, 1, 1)
        halo = r[1] + f[1]
        sh = tiles.empty_shard((4, k), ny, nx, halo, dev)
        sh.ext.fill_(float('nan'))
        sh.core.copy_(full[:, :, sh.r0:sh.r1])
        tiles.exchange_halo_(sh)
        torch.cuda.synchronize()
        assert torch.equal(sh.ext.cpu(), full[:, :, sh.r0 - sh.lo:sh.r1 + sh.hi])
        got_nlm = tiles.nlmeans_rows(sh, ny, r, f, 0.7, 0.9, n_eff=20.0, patch_mode=0)
        got_nlm1 = tiles.nlmeans_rows(sh, ny, (0, 3, 3), (0, 1, 1), 0.7, 0.9, patch_mode=1)
        got_ch = tiles.nlmeans_then_omnibus(sh, ny, r, f, 0.7, 0.9, 0.5, 20, n_eff=20.0)
        shb = tiles.empty_shard((4, k), ny, nx, 2, dev)
        shb.core.copy_(full[:, :, shb.r0:shb.r1])
        got_box = tiles.boxcar_rows(shb, 5)
        torch.cuda.synchronize()
        # every rank computes the unsharded result on its own GPU and compares its rows
        whole = full.to(dev)
        out = torch.empty_like(whole)
        kernels.pixelwise_nlmeans_3d(whole.permute(1, 2, 3, 0), out.permute(1, 2, 3, 0), r, f, 0.7, 0.9,
                                     20.0, patch_mode=0)
        assert torch.equal(got_nlm, out[:, :, sh.r0:sh.r1])
        want_ch = kernels.change_detection(out[0], out[1], out[2], out[3], alpha=0.5, n=20)
        assert torch.equal(got_ch, want_ch[sh.r0:sh.r1])
        assert int(want_ch.sum()) > 0
        out1 = torch.empty_like(whole)
        kernels.pixelwise_nlmeans_3d(whole.permute(2, 3, 1, 0), out1.permute(2, 3, 1, 0), (3, 3, 0),
                                     (1, 1, 0), 0.7, 0.9, -1, patch_mode=1)
        assert torch.equal(got_nlm1, out1[:, :, sh.r0:sh.r1])
        want_box = kernels.convolve(whole, np.ones((1, 1, 5, 5)) / 25.0)
        assert torch.equal(got_box, want_box[:, :, shb.r0:shb.r1])
        ret[rank] = 1
    finally:
        dist.destroy_process_group()


def _run_ranks(world, backend, shared_gpu):
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context('spawn')
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, ret, backend, shared_gpu))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():                       # never leave a rank behind on the GPU box
            p.kill()
            p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert sorted(ret.keys()) == list(range(world))


@needs2
def test_nccl_row_sharded_kernels_equal_unsharded():
    _run_ranks(2, 'nccl', shared_gpu=False)


def test_shared_gpu_row_sharded_kernels_equal_unsharded():
    """Three ranks on ONE GPU (gloo rendezvous, halos staged through the host): interior rank with
    two neighbours, unequal blocks (301 rows -> 101 / 101 / 99)."""
    _run_ranks(3, 'gloo', shared_gpu=True)


@needs2
def test_apply_over_two_devices_equals_one(oracle):
    import torch
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    from nd_amd.filters import BoxcarFilter, NLMeansFilter
    from tests import synth
    planes = synth.omnibus_stack(seed=21, k=10, ny=90, nx=130, dtype=np.float32, change_frac=0.2)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    host = xr_lite.Dataset()
    for v, a in zip(('C11', 'C12__re', 'C12__im', 'C22'), yxt):
        host[v] = (('y', 'x', 'time'), a)
    devs = [0, 1]
    # host dataset
    one = BoxcarFilter(w=5).apply(host)
    two = BoxcarFilter(w=5).apply(host, devices=devs)
    for v in one.data_vars:
        np.testing.assert_array_equal(one[v].values, two[v].values)
    nl1 = NLMeansFilter(dims=('y', 'x'), r=3, f=1, sigma=0.5, h=0.7).apply(host)
    nl2 = NLMeansFilter(dims=('y', 'x'), r=3, f=1, sigma=0.5, h=0.7).apply(host, njobs=2)
    for v in nl1.data_vars:
        np.testing.assert_array_equal(nl1[v].values, nl2[v].values)
    want = oracle.change_detection_planes(yxt, 0.9, 9).astype(bool)
    np.testing.assert_array_equal(OmnibusTest(n=9, alpha=0.9, devices=devs).apply(host).values, want)
    ml1 = OmnibusTest(ml=3, alpha=0.9).apply(host).values
    ml2 = OmnibusTest(ml=3, alpha=0.9, njobs=2).apply(host).values
    np.testing.assert_array_equal(ml1, ml2)
    # the sparse regime, where OmnibusTest(ml=...) takes the FUSED kernel: its 155 KB of dynamic LDS are opted
    # into on every launch, i.e. on every device of the in-process pool (a once-per-process opt-in left the
    # second device without it: ADVICE r04)
    for mlw in (3, 5):
        f1 = OmnibusTest(ml=mlw, alpha=0.99).apply(host).values
        f2 = OmnibusTest(ml=mlw, alpha=0.99, devices=devs).apply(host).values
        np.testing.assert_array_equal(f1, f2)
    # device-resident dataset on GPU 0: chunks travel peer-to-peer, the result comes back to GPU 0
    dev_ds = xr_lite.Dataset()
    for v in host.data_vars:
        dev_ds[v] = (('y', 'x', 'time'), torch.from_numpy(host[v].values).to('cuda:0'))
    two_d = BoxcarFilter(w=5).apply(dev_ds, devices=devs)
    for v in one.data_vars:
        assert two_d[v].values.device == torch.device('cuda:0')
        np.testing.assert_array_equal(two_d[v].values.cpu().numpy(), one[v].values)
    ch = OmnibusTest(n=9, alpha=0.9, devices=devs).apply(dev_ds)
    np.testing.assert_array_equal(ch.values.cpu().numpy(), want)


@needs2
def test_filters_beyond_64_kb_of_lds_on_the_second_device(oracle):
    """The dynamic-LDS limit belongs to a device's function object: a kernel that needs more than 64 KB runs first
    on device 0, then on device 1, and both must give the CPU result bit for bit (the oracle's convolve for the
    window, scipy's correlate1d -- the expectation of the 1-D filter tests -- for the line filter)."""
    import scipy.ndimage as ndi
    import torch
    from nd_amd import kernels
    rng = np.random.default_rng(31)
    a = rng.normal(size=(2, 40, 70)).astype(np.float32)
    box = np.ones((1, 31, 31)) / 961.0             # 62 staged rows of 1280 B plus the index maps: about 79 KB
    want_box = oracle.convolve(a, box)
    # correlate1d along y stages (32 + class - 1) rows of 128 doubles and a 4-byte map entry per row, 1028 B a
    # row: 31 taps (class 31) are 62 rows = 63 736 B; 32 taps, the smallest count beyond 64 KB, take the class
    # of 65: 96 rows = 98 688 B
    w = rng.normal(size=32)
    want_line = ndi.correlate1d(a, w, axis=1)
    for idx in (0, 1):
        t = torch.from_numpy(a).to(torch.device('cuda', idx))
        got_box = kernels.convolve(t, box)
        got_line = kernels.correlate1d(t, w, 1, torch.empty_like(t))
        torch.cuda.synchronize(idx)
        np.testing.assert_array_equal(got_box.cpu().numpy(), want_box, err_msg='device %d' % idx)
        np.testing.assert_array_equal(got_line.cpu().numpy(), want_line, err_msg='device %d' % idx)


def test_devices_argument_with_one_device_is_todays_path(oracle, device):
    """devices=[0] (and njobs=2 on a one-GPU box) degrade to the single-device result."""
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    from nd_amd.filters import BoxcarFilter
    from tests import synth
    planes = synth.omnibus_stack(seed=22, k=8, ny=40, nx=70, dtype=np.float32, change_frac=0.2)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    host = xr_lite.Dataset()
    for v, a in zip(('C11', 'C12__re', 'C12__im', 'C22'), yxt):
        host[v] = (('y', 'x', 'time'), a)
    one = BoxcarFilter(w=3).apply(host)
    for kw in (dict(devices=[0]), dict(njobs=2), dict(njobs=3, devices=[0])):
        two = BoxcarFilter(w=3).apply(host, **kw)
        for v in one.data_vars:
            np.testing.assert_array_equal(one[v].values, two[v].values)
    want = oracle.change_detection_planes(yxt, 0.9, 9).astype(bool)
    np.testing.assert_array_equal(OmnibusTest(n=9, alpha=0.9, devices=[0]).apply(host).values, want)
    np.testing.assert_array_equal(OmnibusTest(n=9, alpha=0.9, njobs=4).apply(host).values, want)


def _bench(args, env, tmp_path, launcher=True, timeout=240):
    """bench.py with two ranks sharing this box's GPU over gloo.  launcher=True: the driver's N > 1 line
    (python -m torch.distributed.run ...); False: plain `python bench.py --gpus 2 ...`, which must start
    the ranks itself.  -> (returncode, result lines, stderr)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ND_AMD_BENCH_REHEARSE='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', **env)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable]
    if launcher:
        cmd += ['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                '--master-addr', '127.0.0.1', '--master-port', str(_free_port())]
    cmd += [os.path.join(root, 'bench.py')] + args
    # output into files, not pipes: a pipe stays open for as long as any descendant of the launcher
    # holds it, and the launcher's exit is what this test waits for
    with open(tmp_path / 'out', 'w') as fo, open(tmp_path / 'err', 'w') as fe:
        p = subprocess.run(cmd, cwd=root, env=env, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                           timeout=timeout)
    stdout, stderr = (tmp_path / 'out').read_text(), (tmp_path / 'err').read_text()
    # gloo announces its connections on stdout, both ranks interleaved (the rehearsal's transport, not
    # bench.py's output; RCCL's banner is silenced in bench.py): everything else is the one JSON line
    banner = set('[Gloo] Rank 0 1 is connected to 1 peer ranks. Expected number of connected peer ranks is : 1')
    lines = [ln for ln in stdout.splitlines() if ln.strip() and not set(ln) <= banner]
    return p.returncode, lines, stderr


@pytest.mark.parametrize('workload,extra', [('omnibus', []), ('omnibus', ['--scaling', 'strong']),
                                            ('pipeline', []), ('c3', [])])
def test_bench_launch_line_with_two_ranks(workload, extra, tmp_path):
    """The driver's N > 1 launch of bench.py (python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 ...), rehearsed with two ranks that share this box's
    GPU over gloo (ND_AMD_BENCH_REHEARSE): row partition per rank, the max-over-ranks time, the
    whole-job pixel count, the halo exchange of the pipeline workload, ONE JSON line from rank 0."""
    import json
    ny, nx, k = (96, 512, 8) if workload != 'pipeline' else (64, 512, 6)
    rc, lines, stderr = _bench(['--gpus', '2', '--steps', '2', '--warmup', '1', '--workload', workload,
                                '--ny', str(ny), '--nx', str(nx), '--k', str(k), '--full'] + extra, {}, tmp_path)
    assert rc == 0, stderr[-3000:]
    assert len(lines) == 1, lines                       # the contract: one JSON line, rank 0 only
    assert len(lines[0].encode()) < 4096
    res = json.loads(lines[0])
    assert res['n_gpus'] == 2 and res['steps'] == 2 and res['warmup'] == 1
    assert res['scaling'] == ('strong' if extra else 'weak')
    assert res['value'] > 0 and res['ms_per_step'] > 0
    total_rows = ny if extra else 2 * ny               # weak: every rank owns `ny` rows
    want = total_rows * nx / (res['ms_per_step'] * 1e-3) / 1e6
    assert abs(res['value'] - want) <= 1e-4 * want      # (the line carries six significant digits)
    assert 'REHEARSAL' in res['data'] and 'roofline' in res
    # the line carries its own evidence of the N > 1 run: one short row per rank
    comm = res['comm']
    assert comm['world_size'] == 2 and comm['backend'] == 'gloo' and len(comm['ranks']) == 2
    assert comm['rank_cols'] == ['rank', 'device_index', 'row0', 'row1', 'step_ms']
    assert [r[0] for r in comm['ranks']] == [0, 1]
    assert comm['device'] and all(r[4] > 0 for r in comm['ranks'])
    rows = [r[2:4] for r in comm['ranks']]
    assert rows[0][0] == 0 and rows[0][1] == rows[1][0] and rows[1][1] == total_rows
    if workload == 'pipeline':
        halo = 4                                            # r_y + f_y of the tutorial's filter
        assert comm['halo_bytes_sent_per_step'] == [4 * k * halo * nx * 4] * 2
        assert all(v > 0 for v in comm['exchange_ms_alone'])
        assert 'p2p' in comm['collective']
        # first contact: the overlapped filter equals the sequential one bit for bit on both ranks
        assert comm['overlap_equals_sequential'] is True and comm['timed_form'] == 'overlapped'
    else:
        assert comm['collective'] == 'none' and 'overlap_equals_sequential' not in comm
    # rank 0 recomputed the rows around the shard boundary unsharded and found them equal
    bc = comm['boundary_check']
    assert bc['boundaries'] == 1 and bc['map_bytes_differing'] == 0 and bc['map_bytes_compared'] > 0
    assert bc['filtered_values_differing'] == (0 if workload == 'pipeline' else None)
    # the long form went to the sidecar file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    det = json.load(open(os.path.join(root, res['detail_file'])))
    assert len(det['comm']['ranks']) == 2 and det['comm']['ranks'][1]['rank'] == 1


def test_bench_gpus_2_starts_two_ranks_by_itself(tmp_path):
    """`python bench.py --gpus 2 ...` with no launcher around it (VERDICT r04 missing 2): two ranks, one
    line with n_gpus: 2 -- never a silent single-rank run."""
    import json
    rc, lines, stderr = _bench(['--gpus', '2', '--steps', '2', '--warmup', '1', '--ny', '96', '--nx', '512',
                                '--k', '8'], {}, tmp_path, launcher=False)
    assert rc == 0, stderr[-3000:]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res['n_gpus'] == 2 and res['comm']['world_size'] == 2
    assert [r[0] for r in res['comm']['ranks']] == [0, 1]


def test_bench_gpus_2_fails_when_a_rank_fails(tmp_path):
    """a rank that dies (here: a raster too small for the filter's halo, every rank raises in
    check_partition) -> non-zero exit of the parent, no result line"""
    rc, lines, stderr = _bench(['--gpus', '2', '--steps', '1', '--warmup', '0', '--workload', 'pipeline',
                                '--scaling', 'strong', '--ny', '6', '--nx', '256', '--k', '4'], {}, tmp_path,
                               launcher=False)
    assert rc != 0
    assert not [ln for ln in lines if ln.lstrip().startswith('{')]
    assert 'smaller than the halo' in stderr


def test_bench_falls_back_to_the_sequential_halo_form(tmp_path):
    """first contact: rank 1's overlapped result is made to differ (test hook) ->
    both ranks time the sequential form, the line says so, and the boundary check is still green."""
    import json
    rc, lines, stderr = _bench(['--gpus', '2', '--steps', '2', '--warmup', '1', '--workload', 'pipeline',
                                '--ny', '64', '--nx', '512', '--k', '6', '--full'],
                               {'ND_AMD_BENCH_FORCE_OVERLAP_DIFF': '1'}, tmp_path)
    assert rc == 0, stderr[-3000:]
    comm = json.loads(lines[-1])['comm']
    assert comm['overlap_equals_sequential'] is False and comm['timed_form'] == 'sequential'
    assert comm['values_differing_max_over_ranks'] == 8
    assert comm['boundary_check']['filtered_values_differing'] == 0
