"""vg_cluster_dbscan on the GPU against vg_dbscan_host (which tests/test_dbscan_host.py holds to the contract and to scikit-learn):
labels, core flags, probabilities and the cluster count equal with no tolerance, on every scene of the fixture in three row orders;
the same bytes on every run and under a captured graph's replay; guard words; handle reuse; the grid left behind; the Python class.
"""

import numpy as np
import pytest

import dbscan_ref as dr
import neighbors_ref as nr
from test_dbscan_host import SCENES, ORDERS, host

pytestmark = pytest.mark.gpu

GUARD = 37
_models = {}


def _model(cuda, eps, ms):
    """the model of (eps, min_samples); the last one is kept, so the orders and repeats of a scene share a handle, as frames do, and
    no more than one handle's tables (a quarter of a gigabyte) stay allocated"""
    from vilgod_amd.dbscan import DBSCAN
    key = (float(eps), int(ms))
    if key not in _models:
        _models.clear()
        _models[key] = DBSCAN(eps=eps, min_samples=ms, max_points=20480, device=cuda)
    return _models[key]


def _device(cuda, X, eps, ms, dim=None, model=None):
    """-> (labels, core, probs, n_clusters) numpy, through DBSCAN.labels_device"""
    import torch
    dim = X.shape[1] if dim is None else dim
    m = model if model is not None else _model(cuda, eps, ms)
    d_labels, d_probs, d_nc, d_core = m.labels_device(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(cuda), dim=dim)
    return d_labels.cpu().numpy(), d_core.cpu().numpy(), d_probs.cpu().numpy(), int(d_nc.item())


def _same(got, want, what):
    for g, w, part in zip(got, want, ('labels', 'core', 'probs', 'n_clusters')):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f'{what}: {part} differ at rows {np.flatnonzero(g != w)[:8]}'
        else:
            assert g == w, f'{what}: {part} {g} != {w}'


@pytest.fixture(scope='module')
def kitti_host():
    """the host twin's answer on the real frame, computed once (1 s)"""
    m, X, _, _ = SCENES('kitti_20000')
    return {order: host(dr.reorder(X, order), m['eps'], m['min_samples']) for order in ORDERS}


@pytest.mark.parametrize('name', [n for n in SCENES.names if n != 'kitti_20000'])
def test_device_equals_host(name, cuda):
    m, X0, _, _ = SCENES(name)
    for order in ORDERS:
        X = dr.reorder(X0, order)
        _same(_device(cuda, X, m['eps'], m['min_samples']), host(X, m['eps'], m['min_samples']), f'{name} {order}')


@pytest.mark.parametrize('order', ORDERS)
def test_real_frame(order, cuda, kitti_host):
    m, X, _, _ = SCENES('kitti_20000')
    _same(_device(cuda, dr.reorder(X, order), m['eps'], m['min_samples']), kitti_host[order], f'kitti {order}')


def test_two_calls_give_identical_bytes(cuda, kitti_host):
    m, X, _, _ = SCENES('kitti_20000')
    first = _device(cuda, X, m['eps'], m['min_samples'])
    again = _device(cuda, X, m['eps'], m['min_samples'])
    _same(again, first, 'second call')
    m, X, _, _ = SCENES('serpentine_ms3')
    first = _device(cuda, X, m['eps'], m['min_samples'])
    for _ in range(3):
        _same(_device(cuda, X, m['eps'], m['min_samples']), first, 'serpentine again')


def test_dim5_then_dim3_on_one_handle(cuda):
    m5, X5, _, _ = SCENES('dim5_points_seq')
    model = _model(cuda, m5['eps'], m5['min_samples'])
    _same(_device(cuda, X5, m5['eps'], m5['min_samples'], model=model), host(X5, m5['eps'], m5['min_samples']), 'dim 5')
    _same(_device(cuda, X5, m5['eps'], m5['min_samples'], dim=3, model=model), host(X5, m5['eps'], m5['min_samples'], 3), 'dim 3 after 5')
    _same(_device(cuda, X5, m5['eps'], m5['min_samples'], dim=4, model=model), host(X5, m5['eps'], m5['min_samples'], 4), 'dim 4 after 3')
    m4, X4, _, _ = SCENES('dim4_two_groups')
    assert _device(cuda, X4, m4['eps'], m4['min_samples'], dim=4)[3] == 2 and _device(cuda, X4, m4['eps'], m4['min_samples'], dim=3)[3] == 1


def test_the_grid_left_behind_serves_a_ball_count(cuda):
    import torch
    m, X, _, _ = SCENES('clamped')
    model = _model(cuda, m['eps'], m['min_samples'])
    d_X = torch.from_numpy(X).to(cuda)
    model.labels_device(d_X)
    r2 = np.float32(0.25)
    counts = model.ball_count(d_X, r2, 1000).cpu().numpy()
    assert np.array_equal(counts, nr.ball_count(X, X, r2, 1000))    # the exact float32 count of tests/test_neighbors_edges.py
    idx, _ = model.nearest(d_X, 1e-12)
    assert np.array_equal(X[idx.cpu().numpy()], X)                   # every row finds itself (or a duplicate) in the grid


@pytest.mark.parametrize('n', [255, 256, 257])
def test_block_size_edges_and_guard_words(n, cuda):
    """n one below, at and one above the kernels' 256-thread block, outputs carved from guarded buffers: no word outside is written"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    rng = np.random.default_rng(n)
    X = (rng.integers(0, 5, (n, 1)) * np.array([[3.0, 0, 0]]) + rng.normal(0, 0.2, (n, 3))).astype(np.float32)
    eps, ms = 0.3, 4
    assert dr.margin(X, eps) > 1e-9
    model = _model(cuda, eps, ms)
    d_X = torch.from_numpy(X).to(cuda)
    bufs = {}
    for key, dtype, fill in (('labels', torch.int32, 0x5A5A5A5A), ('core', torch.uint8, 0xA5), ('probs', torch.float64, -12345.0),
                             ('nc', torch.int32, 0x5A5A5A5A)):
        bufs[key] = torch.full((GUARD + (1 if key == 'nc' else n) + GUARD,), fill, dtype=dtype, device=cuda)
    view = lambda key: bufs[key][GUARD:GUARD + (1 if key == 'nc' else n)]
    rc = lib.vg_cluster_dbscan(model._h, ptr(d_X), n, 3, 3, eps, ms, ptr(view('labels')), ptr(view('core')), ptr(view('probs')),
                               ptr(view('nc')), stream_ptr())
    assert rc == 0
    got = view('labels').cpu().numpy(), view('core').cpu().numpy(), view('probs').cpu().numpy(), int(view('nc').item())
    _same(got, host(X, eps, ms), f'n {n}')
    assert got[3] >= 1
    for key, fill in (('labels', 0x5A5A5A5A), ('core', 0xA5), ('probs', -12345.0), ('nc', 0x5A5A5A5A)):
        b = bufs[key].cpu().numpy()
        assert np.all(b[:GUARD] == fill) and np.all(b[-GUARD:] == fill), key


def test_captured_graph_replays_the_same_bytes(cuda):
    import torch
    m, X, _, _ = SCENES('shared_border')
    model = _model(cuda, m['eps'], m['min_samples'])
    d_X = torch.from_numpy(X).to(cuda)
    want = host(X, m['eps'], m['min_samples'])
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):                                    # warm-up outside the capture
        model.labels_device(d_X)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d_labels, d_probs, d_nc, d_core = model.labels_device(d_X)
    graph.replay()
    torch.cuda.synchronize(cuda)
    _same((d_labels.cpu().numpy(), d_core.cpu().numpy(), d_probs.cpu().numpy(), int(d_nc.item())), want, 'replay')


def test_c_refusals_launch_nothing(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    model = _model(cuda, 0.5, 5)
    n = 8
    d_X = torch.zeros((n, 5), device=cuda)
    out = [torch.full((n,), 77, dtype=torch.int32, device=cuda), torch.full((n,), 77, dtype=torch.uint8, device=cuda),
           torch.full((n,), 77.0, dtype=torch.float64, device=cuda), torch.full((1,), 77, dtype=torch.int32, device=cuda)]

    def call(n=n, stride=5, dim=3, eps=0.5, ms=2, h=model._h):
        return lib.vg_cluster_dbscan(h, ptr(d_X), n, stride, dim, eps, ms, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), stream_ptr())
    for bad in (dict(eps=float('nan')), dict(eps=0.0), dict(eps=-1.0), dict(eps=float(np.nextafter(3.2, 4))), dict(ms=0), dict(dim=2),
                dict(dim=6), dict(n=-1), dict(stride=2), dict(n=model.max_points + 1), dict(h=None)):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize(cuda)
    assert all(bool((o == 77).all()) for o in out)
    assert call(n=0) == 0
    torch.cuda.synchronize(cuda)
    assert int(out[3].item()) == 0 and bool((out[0] == 77).all())      # n == 0: the count alone is written


def test_fit_on_numpy_and_cuda_and_a_side_stream(cuda):
    import torch
    from vilgod_amd.dbscan import DBSCAN
    m, X, labels, core = SCENES('numbering')
    model = _model(cuda, m['eps'], m['min_samples'])
    for arg in (X, torch.from_numpy(X).to(cuda)):
        model.fit(arg)
        assert model.labels_.dtype == np.int64 and np.array_equal(model.labels_, labels)
        assert model.core_sample_indices_.dtype == np.int64 and np.array_equal(model.core_sample_indices_, core)
        assert np.array_equal(model.components_, X[core]) and model.n_clusters_ == 40
        assert np.array_equal(model.probabilities_, (labels >= 0).astype(np.float64))
    m5, X5, l5, _ = SCENES('dim5_points_seq')
    assert np.array_equal(_model(cuda, m5['eps'], m5['min_samples']).fit(X5).labels_, l5)       # numpy: every column counts
    with pytest.raises(ValueError, match='NaN or infinity'):
        model.fit(np.array([[0, 0, np.nan]], np.float32))
    with pytest.raises(NotImplementedError):
        model.fit(np.zeros((4, 2), np.float32))
    with pytest.raises(NotImplementedError):
        model.fit(np.zeros((4, 6), np.float32))
    with pytest.raises(NotImplementedError):
        model.fit(X, sample_weight=np.ones(len(X)))
    side = torch.cuda.Stream(cuda)
    d_X = torch.from_numpy(X).to(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    d_labels, d_probs, d_nc, d_core = model.labels_device(d_X, stream=side)
    side.synchronize()
    assert np.array_equal(d_labels.cpu().numpy(), labels) and int(d_nc.item()) == 40
    assert isinstance(repr(model), str) and 'eps=0.5' in repr(model)
