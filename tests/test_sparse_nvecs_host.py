"""CPU: the nvecs routing of the driver (`init_options.nvecs_method`) against a recording stand-in engine, the
not-converged warning, and the export of `aoadmm_resident_nvecs`."""
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_export_resident_nvecs(pkg):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'aoadmm_hip.h')).read(), flags=re.S)
    assert re.search(r'\baoadmm_resident_nvecs\s*\(', text)
    assert 'aoadmm_nvecs_options' in text and 'aoadmm_nvecs_info' in text
    assert 'aoadmm_resident_nvecs' in pkg.SYMBOLS
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(pkg.load_library(), 'aoadmm_resident_nvecs')


class _Lib:
    def __getattr__(self, name):
        return lambda *a: 0


class _Eng:
    """Stand-in for an Engine: every C call succeeds; uploads and resident_nvecs calls are recorded in order."""
    lib = _Lib()
    h = None

    def __init__(self, converged=1):
        self.log = []
        self.converged = converged
        self._resident_model = 'something else'

    def upload_coo(self, p, subs, vals):
        self.log.append(('upload', p, len(vals)))

    def resident_nvecs(self, p, pos, n, r, **opts):
        self.log.append(('nvecs', p, pos, n, r))
        U = np.zeros((n, r), order='F')
        U[:r, :r] = np.eye(r)
        return U, np.ones(r), dict(iterations=500 if not self.converged else 7, converged=self.converged, block=r,
                                   residual=3.5e-4 if not self.converged else 1e-11, fibers=n)


def _model(pkg, shape=(8, 6, 5), dense=False):
    rng = np.random.default_rng(3)
    X = rng.random(shape)
    X[X < 0.5] = 0
    n = len(shape)
    obj = X if dense else pkg.sptensor(np.argwhere(X), X[X != 0], shape)
    Z = dict(loss_function=['Frobenius'], model=['CP'], modes=[list(range(1, n + 1))], size=list(shape),
             coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
             constrained_modes=[0] * n, constraints=[None] * n, weights=[1.0], object=[obj])
    io = dict(lambdas_init=[[1, 1]], nvecs=1, distr=[lambda a, b: rng.random((a, b))] * n, normalize=1)
    return Z, io, X


def test_automatic_method_keeps_small_sparse_modes_on_the_host(pkg):
    pytest.importorskip('scipy.sparse')
    Z, io, _ = _model(pkg)
    e = _Eng()
    for n in range(3):
        assert pkg.cmtf_nvecs(Z, n, 2, engine=e).shape == (Z['size'][n], 2)
        assert pkg.cmtf_nvecs(Z, n, 2, engine=e, method='gram').shape == (Z['size'][n], 2)
    G = pkg.init_coupled_AOADMM_CMTF(Z, io, rng=np.random.default_rng(0), engine=e)
    assert [f.shape for f in G['fac']] == [(8, 2), (6, 2), (5, 2)]
    assert e.log == []


def test_iterative_method_uploads_once_and_asks_once_per_mode(pkg):
    Z, io, _ = _model(pkg)
    e = _Eng()
    G = pkg.init_coupled_AOADMM_CMTF(Z, {**io, 'nvecs_method': 'iterative'}, rng=np.random.default_rng(0), engine=e)
    assert [x[0] for x in e.log] == ['upload', 'nvecs', 'nvecs', 'nvecs']
    assert sorted(x[2:] for x in e.log[1:]) == [(0, 8, 2), (1, 6, 2), (2, 5, 2)]
    assert all(x[1] == 0 for x in e.log)                   # the scratch model has one block
    assert e._resident_model is None
    assert [f.shape for f in G['fac']] == [(8, 2), (6, 2), (5, 2)]
    e2 = _Eng()
    U = pkg.cmtf_nvecs(Z, 1, 2, engine=e2, method='iterative')      # on its own: its mode only
    assert U.shape == (6, 2) and [x[0] for x in e2.log] == ['upload', 'nvecs'] and e2.log[1][2:] == (1, 6, 2)


def test_automatic_method_takes_long_sparse_modes_to_the_device(pkg, monkeypatch):
    drv = __import__('importlib').import_module('matlab-code_amd.driver')
    assert drv.NVECS_ITERATIVE_ROWS == 16384
    monkeypatch.setattr(drv, 'NVECS_ITERATIVE_ROWS', 7)           # the first mode (8 rows) is now 'long'
    pytest.importorskip('scipy.sparse')
    Z, io, _ = _model(pkg)
    e = _Eng()
    pkg.init_coupled_AOADMM_CMTF(Z, io, rng=np.random.default_rng(0), engine=e)
    assert [x[0] for x in e.log] == ['upload', 'nvecs'] and e.log[1][2:] == (0, 8, 2)


def test_unknown_method_and_dense_block_raise(pkg):
    Z, io, _ = _model(pkg)
    with pytest.raises(ValueError, match='nvecs_method'):
        pkg.cmtf_nvecs(Z, 0, 2, engine=_Eng(), method='lanczos')
    with pytest.raises(ValueError, match='nvecs_method'):
        pkg.init_coupled_AOADMM_CMTF(Z, {**io, 'nvecs_method': 'power'}, rng=np.random.default_rng(0), engine=_Eng())
    Zd, iod, _ = _model(pkg, dense=True)
    e = _Eng()
    with pytest.raises(ValueError, match='sparse blocks only'):
        pkg.cmtf_nvecs(Zd, 0, 2, engine=e, method='iterative')
    assert e.log == []


def test_not_converged_is_a_runtime_warning_with_the_residual(pkg):
    Z, io, _ = _model(pkg)
    with pytest.warns(RuntimeWarning, match=r'500 iterations with residual 3\.500e-04'):
        U = pkg.cmtf_nvecs(Z, 0, 2, engine=_Eng(converged=0), method='iterative')
    assert U.shape == (8, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        pkg.cmtf_nvecs(Z, 0, 2, engine=_Eng(), method='iterative')
