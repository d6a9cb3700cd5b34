"""The wave-search pass A (default) against the two-pass form (ND_AMD_WAVE_SEARCH=0), float32, n = 9: the headline
stack (24 x 4096 x 4096) over alpha, and 8 / 16 / 32 dates on 2048 x 4096 at alpha = 0.99.  Three fresh processes per
form, alternating; maps compared by hash.  (32 dates take the two-pass form under both settings: a control.  So do the
thresholds below kWaveSearchAlpha, omnibus.hip, which was set from this table: lower it there to measure them again;
the `wave_search` column says which form a row ran.)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == 'child':
    sys.path.insert(0, ROOT)
    import time, hashlib, torch
    from nd_amd import synth, kernels, _lib
    dev = torch.device('cuda:0')
    cases = [(24, 4096, 4096, a) for a in (0.93, 0.95, 0.97, 0.99, 0.999)] + [(k, 2048, 4096, 0.99) for k in (8, 16, 32)]
    st, shape = None, None
    for K, ny, nx, alpha in cases:
        if shape != (K, ny, nx):
            st = None
            st = synth.wishart_c2_stack(K, ny, nx, looks=9, seed=1234, device=dev, change_frac=0.01)
            shape = (K, ny, nx)
        fn = lambda: kernels.change_detection(st[0], st[1], st[2], st[3], alpha=alpha, n=9)
        for _ in range(5):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 20 * 1e3
        h = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:10]
        wave = _lib.lib().nd_amd_omnibus_c2_uses_wave_search(0, K, 1, alpha, 9, 0)
        print('k %2d  %d x %d  alpha %-5g  wave_search %d  %.4f ms per call  map %s' % (K, ny, nx, alpha, wave, dt, h), flush=True)
else:
    for rep in range(3):
        for form in ('0', '1'):
            print('repeat %d  ND_AMD_WAVE_SEARCH = %s' % (rep, form), flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], env=dict(os.environ, ND_AMD_WAVE_SEARCH=form),
                           check=True, timeout=240, stdin=subprocess.DEVNULL)
