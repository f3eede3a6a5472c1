"""Host-side mirror of the reference's public interface, running on the HIP engine.

    Zhat, Fac, G, out = cmtf_AOADMM(Z, alg_options=options, init=G|'random', init_options=init)
    G = init_coupled_AOADMM_CMTF(Z, init_options=init[, Delta=...])
    prox, reg = constraints_to_prox(constrained_modes, constraints, sz)

Same names, argument meaning and error behaviour as `functions/cmtf_AOADMM.m:1-206`,
`functions/init_coupled_AOADMM_CMTF.m:1-174` and `functions/constraints_to_prox.m:1-94`.
The structs are Python dicts with the MATLAB field names; `Z['modes']` keeps
MATLAB's 1-based mode numbers and `lin_coupled_modes` its 1-based coupling ids
(0 = uncoupled), so the example scripts translate line by line.

What this layer does is exactly what the MEX gateway does for MATLAB
(`matlab-code_amd/mex/`): validate, turn constraint cells into descriptors,
marshal arrays column-major through the C ABI, run `aoadmm_solve` (which replaces
`cmtf_fun_AOADMM`, cmtf_AOADMM.m:193), and pack `Zhat/Fac/out`.  Features the
device path does not cover raise `UnsupportedOnDevice` so a caller can fall
back to the original MATLAB implementation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi
from .engine import Engine, constraint_descriptor, default_engine
from .ranking import parse_rank_metric
from .sptensor import coo_of, pack_par2_slabs, sptensor
from .sptensor import slab_gram as _sparse_slab_gram
from .sptensor import unfold_gram as _sparse_unfold_gram


def _which_p(Z):
    nb_modes = len(Z['size'])
    out = [None] * nb_modes
    for i in range(nb_modes):
        for p, ms in enumerate(Z['modes']):
            if (i + 1) in list(ms):
                out[i] = p
    if any(v is None for v in out) or max(max(ms) for ms in Z['modes']) != nb_modes:
        raise ValueError('Mismatch between size and modes inputs')     # init_coupled_AOADMM_CMTF.m:32-35
    return out


def constraints_to_prox(constrained_modes, constraints, sz, engine=None):
    """functions/constraints_to_prox.m:1-94 -- returns (prox_operators, reg_func).

    Each prox operator is a callable `(x, rho) -> array` evaluated by the HIP
    kernels (op-level entry `aoadmm_op_prox`); `reg_func` entries are host
    closures (they are only used for reporting).
    """
    eng = engine or default_engine()
    n = len(constrained_modes)
    prox_ops = [None] * n
    reg = [None] * n
    for m in range(n):
        if not constrained_modes[m]:
            continue
        c = constraints[m]
        if c is None or len(c) == 0:
            raise ValueError('No constraint provided for mode %d.' % (m + 1))
        constraint_descriptor(c)     # validates / raises UnsupportedOnDevice
        prox_ops[m] = (lambda x, rho, c=c: eng.prox(c, x, rho))
        name = c[0]
        if name == 'l1 regularization':
            reg[m] = lambda x, eta=c[1]: eta * np.sum(np.abs(x))
        elif name == 'l0 regularization':
            reg[m] = lambda x, eta=c[1]: eta * float(np.count_nonzero(x))
        elif name == 'l2 regularization':
            reg[m] = lambda x, eta=c[1]: eta * np.sum(np.sqrt(np.sum(x * x, axis=0)))
        elif name == 'ridge':
            reg[m] = lambda x, eta=c[1]: eta * np.linalg.norm(x, 'fro') ** 2
        elif name == 'TV regularization':
            reg[m] = lambda x, eta=c[1]: eta * np.sum(x[1:, :] - x[:-1, :])     # quirk of :81 kept
        elif name == 'GL smoothness':
            reg[m] = lambda x, eta=c[1]: eta * np.sum((x[1:, :] - x[:-1, :]) ** 2)
    return prox_ops, reg


def _leading_eigvecs(Y, r):
    """`[U,~] = eigs(Y, r, 'LM')`: eigenvectors of the r eigenvalues of largest magnitude, in that order
    (the sign of each vector is arbitrary, in MATLAB too)."""
    w, V = np.linalg.eigh((Y + Y.T) / 2)
    idx = np.argsort(-np.abs(w), kind='stable')[:r]
    return np.asfortranarray(V[:, idx])


NVECS_ITERATIVE_ROWS = 16384     # a sparse mode with more rows than this starts on the device unless told otherwise


def _nvecs_method(method, sparse, rows):
    """`init_options.nvecs_method` -> 'gram' (Gram matrix of the unfolding + LAPACK) or 'iterative' (subspace iteration
    on the nonzeros, `aoadmm_resident_nvecs`; sparse blocks only).  None: 'iterative' for a sparse block whose mode
    has more than NVECS_ITERATIVE_ROWS rows, 'gram' otherwise."""
    if method is None:
        return 'iterative' if sparse and rows > NVECS_ITERATIVE_ROWS else 'gram'
    if method not in ('gram', 'iterative'):
        raise ValueError("init_options.nvecs_method must be 'gram' or 'iterative', got %r" % (method,))
    if method == 'iterative' and not sparse:
        raise ValueError("nvecs_method 'iterative' handles sparse blocks only (dense blocks take 'gram')")
    return method


def _iterative_nvecs(eng, Z, p, pos, r, state):
    """The r leading left singular vectors of tensor mode `pos` of the sparse block p by `Engine.resident_nvecs`.
    The init runs before build_model, so the block goes up as a scratch one-block model of its own modes with rank r:
    once per block (`state['p']` remembers which block the engine holds), whatever the number of modes asked for."""
    import warnings
    md = [m - 1 for m in Z['modes'][p]]
    if state.get('p') != p:
        n = len(md)
        Zs = dict(loss_function=['Frobenius'], model=[Z['model'][p]], modes=[list(range(1, n + 1))],
                  size=[Z['size'][m] for m in md], weights=[1.0], object=[Z['object'][p]],
                  coupling=dict(lin_coupled_modes=[0] * n, coupling_type=[], coupl_trafo_matrices=[None] * n),
                  constrained_modes=[0] * n, constraints=[None] * n, _ranks=[int(r)] * n)
        state['p'] = None
        build_model(eng, Zs)
        eng._resident_model = None          # a scratch model: not the caller's Z
        state['p'] = p
    U, _, info = eng.resident_nvecs(0, pos, int(Z['size'][md[pos]]), int(r))
    if not info['converged']:
        warnings.warn('nvecs of mode %d: subspace iteration stopped after %d iterations with residual %.3e'
                      % (md[pos] + 1, info['iterations'], info['residual']), RuntimeWarning, stacklevel=3)
    return U


def cmtf_nvecs(Z, n, r, engine=None, method=None, _state=None):
    """functions/cmtf_nvecs.m:1-58 for a CP block: first r left singular vectors of the mode-n unfolding (0-based n)
    of the data set that owns mode n.  method 'gram': the I_n x I_n Gram matrix of the unfolding comes from the device
    (`aoadmm_op_unfold_gram`), or for a sparse block from scipy.sparse on the host (no densified tensor), the r
    leading eigenvectors from LAPACK on the host.  method 'iterative' (sparse blocks): subspace iteration on the
    nonzeros on the device, no Gram matrix (`aoadmm_resident_nvecs`).  None: see `_nvecs_method`."""
    which_p = _which_p(Z)
    p = which_p[n]
    md = [m - 1 for m in Z['modes'][p]]
    coo = coo_of(Z['object'][p])
    how = _nvecs_method(method, coo is not None, int(Z['size'][n]))
    if how == 'iterative':
        # `_state` (init_coupled_AOADMM_CMTF): while block p is on the device, every mode it owns that takes this path
        # is computed, so a block coupled with others still goes up once however the modes interleave
        st = {} if _state is None else _state
        cache = st.setdefault('U', {})
        if (n, r) not in cache:
            eng = engine or default_engine()
            for m in md:
                if m == n or (_state is not None and which_p[m] == p and (m, r) not in cache
                              and _nvecs_method(method, True, int(Z['size'][m])) == 'iterative'):
                    cache[(m, r)] = _iterative_nvecs(eng, Z, p, md.index(m), r, st)
        return cache[(n, r)]
    if coo is not None:             # sparse block: sptenmat(X, n) * sptenmat(X, n)' on the host (cmtf_nvecs.m:41-42)
        return _leading_eigvecs(_sparse_unfold_gram(*coo, md.index(n)), r)
    eng = engine or default_engine()
    Y = _resident_gram(eng, Z, p, md.index(n), int(Z['size'][n]))
    if Y is None:
        Y = eng.unfold_gram(np.asarray(Z['object'][p], dtype=np.float64), md.index(n))
    return _leading_eigvecs(Y, r)


def _resident_gram(eng, Z, p, pos, n, slab=0):
    """Gram matrix of an unfolding from the data `build_model(eng, Z)` already put on the device (cmtf_nvecs.m unfolds the
    array it already holds: no second transfer of the tensor); None when this Z is not the engine's resident model or
    the engine cannot answer locally (first mode of a row-sharded block)."""
    if getattr(eng, '_resident_model', None) is not Z:
        return None
    try:
        return eng.resident_unfold_gram(p, pos, n, slab)
    except capi.UnsupportedOnDevice:
        return None


def _par2_sparse(slabs, p):
    """True when every slab of a PARAFAC2 block is sparse (sptensor / .tocoo()), False when every slab is dense."""
    kinds = [coo_of(Xk) is not None for Xk in slabs]
    if any(kinds) and not all(kinds):
        raise ValueError('Z.object{%d}: the slabs of a PARAFAC2 block must be all sparse or all dense' % (p + 1))
    return bool(kinds) and all(kinds)


def init_coupled_AOADMM_CMTF(Z, init_options, Delta=None, rng=None, engine=None):
    """functions/init_coupled_AOADMM_CMTF.m:1-174: random initialisation (`nvecs = 0`) or SVD-based (`nvecs = 1`,
    :50-73), the latter with the unfolding Gram matrices computed on the device."""
    if rng is None:
        rng = np.random.default_rng()
    nvecs = bool(init_options.get('nvecs', 0))
    eng_nv = (engine or default_engine()) if nvecs else None
    nv_method = init_options.get('nvecs_method')     # None: automatic (see _nvecs_method)
    nv_state = {}                                    # which block the engine holds as a scratch model ('iterative')
    sz = Z['size']
    lambdas = init_options['lambdas_init']
    distr = init_options['distr']
    normalize = init_options['normalize']
    nb_modes = len(sz)
    _which_p(Z)
    lin = [int(v) for v in Z['coupling']['lin_coupled_modes']]
    nb_couplings = max(lin) if lin else 0
    ctm = Z['coupling'].get('coupl_trafo_matrices', [None] * nb_modes)
    P = len(Z['modes'])
    A = {'fac': [None] * nb_modes, 'coupling_fac': [None] * nb_couplings, 'constraint_fac': [None] * nb_modes,
         'coupling_dual_fac': [None] * nb_modes, 'constraint_dual_fac': [None] * nb_modes,
         'DeltaB': {}, 'P': {}, 'mu_DeltaB': {}}

    def colnorm(M):
        return M / np.sqrt(np.sum(M * M, axis=0))[None, :]

    for p in range(P):
        md = [m - 1 for m in Z['modes'][p]]
        R = len(lambdas[p])
        for n in md:
            if nvecs:                                                           # :50-73
                if Z['model'][p] == 'CP':
                    A['fac'][n] = cmtf_nvecs(Z, n, R, eng_nv, nv_method, nv_state)
                elif md.index(n) == 0:
                    sparse_slabs = _par2_sparse(Z['object'][p], p)
                    if _nvecs_method(nv_method, sparse_slabs, int(sz[n])) == 'iterative':   # Xcat Xcat' on the device
                        A['fac'][n] = _iterative_nvecs(eng_nv, Z, p, 0, R, nv_state)
                        continue
                    if sparse_slabs:                        # sum_k X_k X_k' on the host, no densified slab
                        Y = sum(_sparse_slab_gram(Xk, 0) for Xk in Z['object'][p])
                    else:
                        Y = _resident_gram(eng_nv, Z, p, 0, int(sz[n]))
                    if Y is None:
                        M = np.hstack([np.asarray(Xk, dtype=np.float64) for Xk in Z['object'][p]])
                        Y = eng_nv.unfold_gram(M, 0)
                    A['fac'][n] = _leading_eigvecs(Y, R)
                elif md.index(n) == 1:
                    A['DeltaB'][p] = rng.random((R, R))
                    A['fac'][n] = []
                    A['P'][p] = []
                    A['mu_DeltaB'][p] = []
                    sparse_slabs = _par2_sparse(Z['object'][p], p)
                    for k in range(len(sz[n])):
                        if sparse_slabs:
                            Y = _sparse_slab_gram(Z['object'][p][k], 1)
                        else:
                            Y = _resident_gram(eng_nv, Z, p, 1, int(sz[n][k]), k)
                        if Y is None:
                            Y = eng_nv.unfold_gram(np.asarray(Z['object'][p][k], dtype=np.float64), 1)
                        A['fac'][n].append(_leading_eigvecs(Y, R))
                        A['P'][p].append(np.eye(sz[n][k], R))
                        A['mu_DeltaB'][p].append(rng.random((sz[n][k], R)))
                else:
                    A['fac'][n] = np.ones((sz[n], R))
                continue
            if Z['model'][p] == 'PAR2' and md.index(n) == 1:
                A['DeltaB'][p] = rng.random((R, R))
                A['fac'][n] = []
                A['P'][p] = []
                A['mu_DeltaB'][p] = []
                for k in range(len(sz[n])):
                    F = np.asarray(distr[n](sz[n][k], R), dtype=np.float64)
                    A['P'][p].append(np.eye(sz[n][k], R))
                    A['mu_DeltaB'][p].append(rng.random((sz[n][k], R)))
                    A['fac'][n].append(colnorm(F) if normalize else F)
            else:
                F = np.asarray(distr[n](sz[n], R), dtype=np.float64)
                A['fac'][n] = colnorm(F) if normalize else F
    if any(Z['constrained_modes']):
        prox_ops, _ = constraints_to_prox(Z['constrained_modes'], Z['constraints'], sz, engine)
        for p in range(P):
            md = [m - 1 for m in Z['modes'][p]]
            for n in md:
                if not Z['constrained_modes'][n]:
                    continue
                if Z['model'][p] == 'PAR2' and md.index(n) == 1:
                    A['constraint_fac'][n] = []
                    A['constraint_dual_fac'][n] = []
                    for k in range(len(sz[n])):
                        Zk = np.asarray(distr[n](*A['fac'][n][k].shape), dtype=np.float64)
                        if Z['constraints'][n][0] != 'tPARAFAC2':
                            Zk = prox_ops[n](Zk, 1.0)
                        A['constraint_fac'][n].append(Zk)
                        A['constraint_dual_fac'][n].append(rng.random(A['fac'][n][k].shape))
                else:
                    if Z['constraints'][n][0] == 'tPARAFAC2':
                        raise ValueError('The tPARAFAC2 constraint can only be impsed on the second mode of a PARAFAC2 model')
                    Zn = np.asarray(distr[n](*A['fac'][n].shape), dtype=np.float64)
                    A['constraint_fac'][n] = prox_ops[n](Zn, 1.0)
                    A['constraint_dual_fac'][n] = rng.random(A['fac'][n].shape)
    for n in range(nb_couplings):
        cmodes = [i for i, v in enumerate(lin) if v == n + 1]
        mode1 = cmodes[0]
        ct = int(Z['coupling']['coupling_type'][n])
        F1 = A['fac'][mode1]
        if ct == 0:
            A['coupling_fac'][n] = rng.random(F1.shape)
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random(A['coupling_fac'][n].shape)
        elif ct == 1:
            A['coupling_fac'][n] = rng.random((ctm[mode1].shape[0], F1.shape[1]))
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random(A['coupling_fac'][n].shape)
        elif ct == 2:
            A['coupling_fac'][n] = rng.random((F1.shape[0], ctm[mode1].shape[1]))
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random(A['coupling_fac'][n].shape)
        elif ct == 3:
            A['coupling_fac'][n] = rng.random((ctm[mode1].shape[1], F1.shape[1]))
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random(A['fac'][m].shape)
        elif ct == 4:
            A['coupling_fac'][n] = rng.random((F1.shape[0], ctm[mode1].shape[0]))
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random(A['fac'][m].shape)
        else:
            A['coupling_fac'][n] = rng.random(np.shape(Delta[n]))
            for m in cmodes:
                A['coupling_dual_fac'][m] = rng.random((A['coupling_fac'][n].shape[0], A['fac'][m].shape[1]))
    return A


def _make_options(alg_options):
    o = capi.Options()
    for name in ('MaxOuterIters', 'MaxInnerIters', 'AbsFuncTol', 'OuterRelTol', 'innerRelPrTol_coupl',
                 'innerRelPrTol_constr', 'innerRelDualTol_coupl', 'innerRelDualTol_constr', 'bsum'):
        if name not in alg_options:
            raise KeyError("Reference to non-existent field '%s'." % name)   # MATLAB: missing option field errors
        setattr(o, name, alg_options[name])
    o.bsum = int(bool(alg_options['bsum']))
    if o.bsum:
        o.bsum_weight = float(alg_options['bsum_weight'])
    o.iter_start_PAR2Bkconstraint = int(alg_options.get('iter_start_PAR2Bkconstraint', 0))   # cmtf_fun_AOADMM.m:7-9
    if 'increase_factor_rhoBk' in alg_options:
        o.has_increase_factor_rhoBk = 1
        o.increase_factor_rhoBk = float(alg_options['increase_factor_rhoBk'])
    hip = alg_options.get('hip', {})
    o.use_dimtree = int(hip.get('use_dimtree', 1))
    o.no_permuted_copy = int(hip.get('no_permuted_copy', 0))
    o.par2_slab_sharding = int(hip.get('par2_slab_sharding', 0))
    o.heldout_patience = int(hip.get('heldout_patience', 0))
    return o


def _unsupported(msg):
    return capi.UnsupportedOnDevice(capi.ERR_UNSUPPORTED, msg)


def observed_only_blocks(Z, observed_only, sparse_sharding=False):
    """The 0-based blocks that `alg_options['hip']['sparse_observed_only']` marks: 0 / None / False -> none, 1 / True ->
    every sparse CP block, a list -> those 1-based blocks, each of which must be a sparse CP block.  Raises
    `UnsupportedOnDevice` for a dense block, a PAR2 block and for any marked block together with `sparse_sharding`."""
    P = len(Z['object'])

    def sparse_cp(p):
        obj = Z['object'][p]
        return Z['model'][p] == 'CP' and not isinstance(obj, dict) and coo_of(obj) is not None

    if observed_only is None or isinstance(observed_only, (bool, int, np.integer)):
        if observed_only is None or int(observed_only) == 0:
            return []
        if int(observed_only) != 1:
            raise ValueError('sparse_observed_only must be 0, 1 or a list of 1-based block numbers')
        blocks = [p for p in range(P) if sparse_cp(p)]
    else:
        blocks = []
        for q in observed_only:
            p = int(q) - 1
            if int(q) != q or p < 0 or p >= P:
                raise ValueError('sparse_observed_only names Z.object{%s}: the model has %d blocks' % (q, P))
            if Z['model'][p] != 'CP':
                raise _unsupported('sparse_observed_only: Z.object{%d} is a PARAFAC2 block (sparse slabs with missing '
                                   'entries are not supported)' % (p + 1))
            if not sparse_cp(p):
                raise _unsupported('sparse_observed_only: Z.object{%d} is dense (use Z.miss for a dense block)' % (p + 1))
            if p not in blocks:
                blocks.append(p)
    if blocks and sparse_sharding:
        raise _unsupported('sparse_observed_only is not available together with sparse_sharding: an observed-only '
                           'block is replicated')
    return blocks


def missing_list_blocks(Z, missing_list, dense_weighted=(), world=1):
    """The 0-based blocks that `alg_options['hip']['missing_list']` marks (`Engine.set_missing_list`): 0 / None / False ->
    none, 1 / True -> every dense CP block with Z.miss that carries no entry weights, a list -> those 1-based blocks, each
    of which must be such a block.  Checked on the host before anything is uploaded.  Raises `UnsupportedOnDevice` for a
    PAR2 block, a sparse block, a block named in `entry_weights` as well (`dense_weighted`: the blocks `dense_weight_blocks`
    returned) and for any marked block on an engine whose communicator has `world` > 1 ranks; ValueError for a block
    without Z.miss."""
    P = len(Z['object'])
    miss = Z.get('miss') if Z.get('miss') is not None else [None] * P

    def dense_masked_cp(p):
        obj = Z['object'][p]
        return Z['model'][p] == 'CP' and not isinstance(obj, dict) and coo_of(obj) is None and miss[p] is not None

    if missing_list is None or isinstance(missing_list, (bool, int, np.integer)):
        if missing_list is None or int(missing_list) == 0:
            return []
        if int(missing_list) != 1:
            raise ValueError('missing_list must be 0, 1 or a list of 1-based block numbers')
        blocks = [p for p in range(P) if dense_masked_cp(p) and p not in dense_weighted]
    else:
        blocks = []
        for q in missing_list:
            p = int(q) - 1
            if int(q) != q or p < 0 or p >= P:
                raise ValueError('missing_list names Z.object{%s}: the model has %d blocks' % (q, P))
            if Z['model'][p] != 'CP':
                raise _unsupported('missing_list: Z.object{%d} is a PARAFAC2 block' % (p + 1))
            if not isinstance(Z['object'][p], dict) and coo_of(Z['object'][p]) is not None:
                raise _unsupported('missing_list: Z.object{%d} is sparse (use sparse_observed_only)' % (p + 1))
            if p in dense_weighted:
                raise _unsupported('missing_list: Z.object{%d} carries entry_weights (a weighted block has no mask)' % (p + 1))
            if not dense_masked_cp(p):
                raise ValueError('missing_list: Z.object{%d} has no Z.miss{%d}' % (p + 1, p + 1))
            if p not in blocks:
                blocks.append(p)
    if blocks and world > 1:
        raise _unsupported('missing_list is not available under a communicator of %d ranks' % world)
    return blocks


def entry_weight_blocks(Z, entry_weights, unstored_weight, observed=(), sparse_sharding=False):
    """`alg_options['hip']['sparse_entry_weights']` / `['sparse_unstored_weight']` -> {0-based block: (wts or None,
    alpha)}, checked on the host before the engine is touched.  Each option is None or a list over the blocks:
    `entry_weights[p]` is an array aligned with the `subs` / `vals` of Z.object{p} as an `sptensor` (or with the
    entries `.tocoo()` returns), or None for stored weights 1; `unstored_weight[p]` is alpha for block p, or None.
    `unstored_weight` may be one number: the alpha of every block named in `entry_weights` and of every block in
    `observed` (the blocks `sparse_observed_only` marks).  A block named in either list is weighted (and marked
    observed-only); its alpha defaults to 0.  ValueError: a list of another length than Z.object, a length mismatch
    with the stored entries, a weight or alpha that is not finite or lies outside [0, 1].  `UnsupportedOnDevice`: a dense
    block, a PAR2 block, and any weighted block together with `sparse_sharding`."""
    P = len(Z['object'])
    if entry_weights is None and unstored_weight is None:
        return {}
    scalar = unstored_weight is not None and not isinstance(unstored_weight, (list, tuple, np.ndarray))
    if entry_weights is not None and (not isinstance(entry_weights, (list, tuple)) or len(entry_weights) != P):
        raise ValueError('sparse_entry_weights must be a list over the %d blocks of Z.object' % P)
    if unstored_weight is not None and not scalar and len(unstored_weight) != P:
        raise ValueError('sparse_unstored_weight must be one number or a list over the %d blocks of Z.object' % P)
    named = [p for p in range(P) if (entry_weights is not None and entry_weights[p] is not None) or
             (unstored_weight is not None and not scalar and unstored_weight[p] is not None)]
    if scalar:
        named = sorted(set(named) | set(observed))
    out = {}
    for p in named:
        obj = Z['object'][p]
        if Z['model'][p] != 'CP':
            raise _unsupported('sparse_entry_weights: Z.object{%d} is a PARAFAC2 block (weights on sparse slabs are not '
                               'supported)' % (p + 1))
        coo = None if isinstance(obj, dict) else coo_of(obj)
        if coo is None:
            raise _unsupported('sparse_entry_weights: Z.object{%d} is dense (weights are for sparse CP blocks; a dense block '
                               'takes entry_weights)' % (p + 1))
        alpha = unstored_weight if scalar else (None if unstored_weight is None else unstored_weight[p])
        alpha = 0.0 if alpha is None else float(alpha)
        if not (np.isfinite(alpha) and 0.0 <= alpha <= 1.0):
            raise ValueError('sparse_unstored_weight: %r for Z.object{%d} is outside [0, 1] (divide the weights by their '
                             'maximum)' % (alpha, p + 1))
        w = None
        if entry_weights is not None and entry_weights[p] is not None:
            w = np.ascontiguousarray(np.asarray(entry_weights[p], dtype=np.float64).reshape(-1))
            if w.shape[0] != len(coo[1]):
                raise ValueError('sparse_entry_weights{%d}: %d weights for %d stored entries' % (p + 1, w.shape[0], len(coo[1])))
            if not (np.all(np.isfinite(w)) and np.all(w >= 0.0) and np.all(w <= 1.0)):
                raise ValueError('sparse_entry_weights{%d}: a weight is outside [0, 1] (divide the weights by their '
                                 'maximum)' % (p + 1))
        out[p] = (w, alpha)
    if out and sparse_sharding:
        raise _unsupported('sparse_entry_weights is not available together with sparse_sharding: a weighted block is '
                           'replicated')
    return out


def dense_weight_blocks(Z, entry_weights):
    """`alg_options['hip']['entry_weights']` -> {0-based block: W (float64, column-major) as it goes to
    `Engine.tensor_weights_upload`}, checked on the host before the engine is touched.  The option is None or a list over
    the blocks holding None or an array of the block's shape with entries in [0, 1]; with Z.miss{p} as well the block's
    weights are W o miss and no mask is uploaded (w = 0 is the spelling of "missing").  ValueError: a list of another
    length than Z.object, a wrong shape, a weight that is not finite or lies outside [0, 1].  `UnsupportedOnDevice`: a
    PAR2 block, and a sparse block (its weights are `sparse_entry_weights`)."""
    P = len(Z['object'])
    if entry_weights is None:
        return {}
    if not isinstance(entry_weights, (list, tuple)) or len(entry_weights) != P:
        raise ValueError('entry_weights must be a list over the %d blocks of Z.object' % P)
    miss = Z.get('miss') if Z.get('miss') is not None else [None] * P
    out = {}
    for p in range(P):
        if entry_weights[p] is None:
            continue
        obj = Z['object'][p]
        if Z['model'][p] != 'CP':
            raise _unsupported('entry_weights: Z.object{%d} is a PARAFAC2 block (weights are for dense CP blocks, and for '
                               'sparse ones through sparse_entry_weights)' % (p + 1))
        if isinstance(obj, dict):
            raise ValueError('entry_weights needs explicit data in Z.object{%d}' % (p + 1))
        if coo_of(obj) is not None:
            raise _unsupported('entry_weights: Z.object{%d} is sparse (use sparse_entry_weights / sparse_unstored_weight)'
                               % (p + 1))
        W = np.asarray(entry_weights[p], dtype=np.float64)
        if tuple(W.shape) != tuple(np.shape(obj)):
            raise ValueError('entry_weights{%d} has size %s, Z.object{%d} has %s' % (p + 1, tuple(W.shape), p + 1,
                                                                                  tuple(np.shape(obj))))
        if not (np.all(np.isfinite(W)) and np.all(W >= 0.0) and np.all(W <= 1.0)):
            raise ValueError('entry_weights{%d}: a weight is outside [0, 1] (divide the weights by their maximum)' % (p + 1))
        if miss[p] is not None:
            mk = np.asarray(miss[p])
            if tuple(mk.shape) != tuple(W.shape):
                raise ValueError('Z.miss{%d} size does not match Z.object{%d}.' % (p + 1, p + 1))
            W = W * (mk != 0)
        out[p] = np.asfortranarray(W)
    return out


def heldout_lists(Z, heldout, patience=0):
    """`alg_options['hip']['heldout']` -> {0-based block: (subs n x N int64 0-based, vals n float64)}, checked on the
    host before the engine is touched.  `heldout` maps 1-based block numbers to `(subs, vals)` or to an `sptensor` of the
    block's size (its stored entries are the list); None / {} -> no list.  For a PAR2 block the subscripts are
    (i, j within slab k, k).  ValueError: a block the model does not have, subs that are not n x N, not integers or out
    of range, len(vals) != n, a value that is not finite, and `patience` > 0 (or not a non-negative integer) without
    any list."""
    P = len(Z['object'])
    if patience is None or isinstance(patience, bool) or int(patience) != patience or int(patience) < 0:
        raise ValueError('heldout_patience must be a non-negative integer, got %r' % (patience,))
    lists = {}
    if heldout is not None and not isinstance(heldout, dict):
        raise ValueError('heldout must be a dict {1-based block number: (subs, vals) or sptensor}')
    for q, item in (heldout or {}).items():
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 1 or q > P:
            raise ValueError('heldout names Z.object{%s}: the model has %d blocks' % (q, P))
        p = int(q) - 1
        md = [m - 1 for m in Z['modes'][p]]
        par2 = Z['model'][p] == 'PAR2'
        shape = [int(Z['size'][md[0]]), None, int(Z['size'][md[2]])] if par2 else [int(Z['size'][m]) for m in md]
        if isinstance(item, sptensor):
            if par2 or tuple(item.shape) != tuple(shape):
                raise ValueError('heldout{%d}: an sptensor must have the size of the CP block Z.object{%d}' % (q, q))
            subs, vals = item.subs, item.vals
        else:
            try:
                subs, vals = item
            except (TypeError, ValueError):
                raise ValueError('heldout{%d} must be (subs, vals) or an sptensor' % q) from None
        subs = np.asarray(subs)
        vals = np.asarray(vals, dtype=np.float64).reshape(-1)
        if subs.ndim != 2 or subs.shape[1] != len(md):
            raise ValueError('heldout{%d}: subs must be n x %d, got %s' % (q, len(md), subs.shape))
        if subs.shape[0] != vals.shape[0]:
            raise ValueError('heldout{%d}: %d subscripts but %d values' % (q, subs.shape[0], vals.shape[0]))
        if not np.issubdtype(subs.dtype, np.integer):
            if not (np.issubdtype(subs.dtype, np.floating) and np.all(np.isfinite(subs)) and np.all(subs == np.floor(subs))):
                raise ValueError('heldout{%d}: subscripts must be integers' % q)
        subs = subs.astype(np.int64)
        if not np.all(np.isfinite(vals)):
            raise ValueError('heldout{%d}: a value is not finite' % q)
        for m in range(len(md)):
            if par2 and m == 1:
                continue
            if subs.shape[0] and (subs[:, m].min() < 0 or subs[:, m].max() >= shape[m]):
                raise ValueError('heldout{%d}: a subscript of mode %d is outside [0, %d)' % (q, m + 1, shape[m]))
        if par2 and subs.shape[0]:
            Jk = np.asarray([int(v) for v in Z['size'][md[1]]], dtype=np.int64)
            if subs[:, 1].min() < 0 or np.any(subs[:, 1] >= Jk[subs[:, 2]]):
                raise ValueError('heldout{%d}: a subscript of mode 2 is outside its slab' % q)
        if subs.shape[0]:
            lists[p] = (np.ascontiguousarray(subs), np.ascontiguousarray(vals))
    if int(patience) > 0 and not lists:
        raise ValueError('heldout_patience = %d needs a held-out list (alg_options.hip.heldout)' % int(patience))
    return lists


def rank_options(Z, hip, heldout_patience=0):
    """`alg_options['hip']['rank_lists']`, `['rank_metric']`, `['rank_every']`, `['rank_patience']`, `['rank_criterion']` ->
    dict(lists={0-based block: (mode 0-based, subs nq x N int64 0-based, exclude or None)}, metric, k, every, patience,
    criterion), checked on the host before the engine is touched.  `rank_lists` maps 1-based block numbers of CP blocks
    to dict(mode=1-based position in the block, subs=nq x N 0-based with the target in that column, exclude=(off, idx) or
    None); None / {} -> no list.  ValueError: a block the model does not have or a PAR2 block, a mode outside the block,
    subs that are not nq x N integers in range, exclusion lists that do not match nq or hold rows out of range, a metric
    string `parse_rank_metric` refuses, every < 1, patience < 0, a criterion that is neither 0 nor 1, patience > 0
    without criterion = 1, and criterion = 1 without a list or together with heldout_patience > 0."""
    P = len(Z['object'])
    spec = hip.get('rank_lists')
    if spec is not None and not isinstance(spec, dict):
        raise ValueError('rank_lists must be a dict {1-based block number: dict(mode=, subs=, exclude=)}')

    def integer(name, lo, default):
        v = hip.get(name, default)
        if isinstance(v, (bool, np.bool_)):
            v = int(v)
        try:
            ok = not isinstance(v, (str, bytes)) and int(v) == v and int(v) >= lo
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('%s must be an integer >= %d, got %r' % (name, lo, v))
        return int(v)

    metric, k = parse_rank_metric(hip.get('rank_metric', 'ndcg@10'))
    every = integer('rank_every', 1, 1)
    patience = integer('rank_patience', 0, 0)
    criterion = integer('rank_criterion', 0, 0)
    if criterion not in (0, 1):
        raise ValueError('rank_criterion must be 0 or 1, got %r' % (criterion,))
    if patience > 0 and criterion != 1:
        raise ValueError('rank_patience = %d needs rank_criterion = 1' % patience)
    lists = {}
    for q, item in (spec or {}).items():
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 1 or q > P:
            raise ValueError('rank_lists names Z.object{%s}: the model has %d blocks' % (q, P))
        p = int(q) - 1
        if Z['model'][p] == 'PAR2':
            raise ValueError('rank_lists{%d}: ranking lists are for CP blocks, Z.object{%d} is a PARAFAC2 block' % (q, q))
        if not isinstance(item, dict) or 'mode' not in item or 'subs' not in item:
            raise ValueError('rank_lists{%d} must be dict(mode=, subs=, exclude=)' % q)
        md = [m - 1 for m in Z['modes'][p]]
        shape = [int(Z['size'][m]) for m in md]
        mode = item['mode']
        if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or mode < 1 or mode > len(md):
            raise ValueError('rank_lists{%d}: mode %r outside [1, %d]' % (q, mode, len(md)))
        mode = int(mode) - 1
        subs = np.asarray(item['subs'])
        if subs.ndim != 2 or subs.shape[1] != len(md):
            raise ValueError('rank_lists{%d}: subs must be nq x %d, got %s' % (q, len(md), subs.shape))
        if not np.issubdtype(subs.dtype, np.integer):
            if not (np.issubdtype(subs.dtype, np.floating) and np.all(np.isfinite(subs)) and np.all(subs == np.floor(subs))):
                raise ValueError('rank_lists{%d}: subscripts must be integers' % q)
        subs = np.ascontiguousarray(subs.astype(np.int64))
        nq = subs.shape[0]
        for m in range(len(md)):
            if nq and (subs[:, m].min() < 0 or subs[:, m].max() >= shape[m]):
                raise ValueError('rank_lists{%d}: a subscript of mode %d is outside [0, %d)' % (q, m + 1, shape[m]))
        exclude = item.get('exclude')
        if exclude is not None:
            try:
                off, idx = exclude
            except (TypeError, ValueError):
                raise ValueError('rank_lists{%d}: exclude must be (off, idx)' % q) from None
            off = np.ascontiguousarray(np.asarray(off, dtype=np.int64).reshape(-1))
            idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
            if off.shape[0] != nq + 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != idx.shape[0]:
                raise ValueError('rank_lists{%d}: exclude[0] must hold nq + 1 = %d non-decreasing offsets from 0 to len(exclude[1])' % (q, nq + 1))
            if idx.shape[0] and (idx.min() < 0 or idx.max() >= shape[mode]):
                raise ValueError('rank_lists{%d}: an excluded row is outside [0, %d)' % (q, shape[mode]))
            exclude = (off, idx)
        if nq:
            lists[p] = (mode, subs, exclude)
    if criterion == 1 and not lists:
        raise ValueError('rank_criterion = 1 needs a ranking list (alg_options.hip.rank_lists)')
    if criterion == 1 and int(heldout_patience) > 0:
        raise ValueError('rank_criterion = 1 and heldout_patience = %d: one rule selects the model' % int(heldout_patience))
    return dict(lists=lists, metric=metric, k=k, every=every, patience=patience, criterion=criterion)


def heldout_keep_best_option(value, lists):
    """`alg_options['hip']['heldout_keep_best']` -> 0 or 1, checked on the host before the engine is touched.  ValueError:
    a value that is not an integer or is neither 0 nor 1 (True / False count), and 1 without a held-out list (`lists`
    as `heldout_lists` returns them)."""
    if isinstance(value, (bool, np.bool_)):
        value = int(value)
    try:
        ok = not isinstance(value, (str, bytes)) and int(value) == value and int(value) in (0, 1)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('heldout_keep_best must be 0 or 1, got %r' % (value,))
    if int(value) == 1 and not lists:
        raise ValueError('heldout_keep_best = 1 needs a held-out list (alg_options.hip.heldout)')
    return int(value)


def build_model(eng, Z, precision='f64', sparse_sharding=False, observed_only=0, entry_weights=None, unstored_weight=None,
                dense_entry_weights=None, missing_list=0):
    """Describe the struct Z to the engine and upload Z.object (cmtf_AOADMM.m:23-41,124-156).

    Z.object{p} of a CP block may be dense, an `sptensor`, or (2-way blocks) any object with `.tocoo()` such as a
    scipy.sparse matrix; sparse blocks go up as coalesced COO nonzeros (`aoadmm_tensor_upload_coo`) and stay fp64
    whatever `precision` says (it applies to dense blocks only).  `precision` is 'f64', 'f32' or 'f16'; with 'f16'
    every dense 3-way CP block without Z.miss is stored as fp16 with one power-of-two scale (AOADMM_PREC_F16,
    `capi.quantize_f16` is the rule) and every other dense block as fp32.  On an engine that belongs to a communicator
    (`Engine.comm_init_*`) the 'f16' upload of such a block is a COLLECTIVE: every rank calls `build_model` with the same
    whole array, keeps its rows (and its mode-3 slab) as fp16 and gets the scale of the WHOLE tensor; a non-finite entry
    anywhere raises `AoadmmError` (ERR_INVALID) on every rank.  A multi-device engine (`Engine([0, 1, ...])`) answers 'f16'
    with `UnsupportedOnDevice`.  The slabs of a PAR2 block may likewise be 2-way
    `sptensor`s or objects with `.tocoo()`, all of them or none (`aoadmm_par2_slab_upload_coo`).
    sparse_sharding: sparse CP blocks go up through `aoadmm_tensor_upload_coo_sharded`, so that every rank of the
    engine's communicator (or every engine of a multi-device one) keeps its share of the nonzeros and the block's
    MTTKRPs become all-reduces; every rank calls `build_model` with the same Z.  PAR2 blocks with sparse slabs stay
    replicated.
    observed_only (`observed_only_blocks`: 0, 1 or a list of 1-based block numbers): the named sparse CP blocks are
    marked observed-only after their upload (`Engine.set_observed_only`): their stored entries are the observations,
    every other entry is missing and fitted by EM as Z.miss does for dense data.  Z.miss on a sparse block keeps
    raising the reference's error.
    entry_weights, unstored_weight (`entry_weight_blocks`): weighted least squares on the named sparse CP blocks
    (`Engine.set_entry_weights`): a weight in [0, 1] for every stored entry and one for all unstored entries.  A named
    block is marked observed-only as well.
    dense_entry_weights (`dense_weight_blocks`): weighted least squares on the named DENSE CP blocks
    (`Engine.tensor_weights_upload`): a list over the blocks, or the dict `dense_weight_blocks` made of it; a block with Z.miss as well
    gets W o miss as weights and no mask.  Under 'f16' such a block goes up as fp32, like a masked one.
    missing_list (`missing_list_blocks`: 0, 1 or a list of 1-based block numbers): the named dense CP blocks with Z.miss
    are marked after their mask is uploaded (`Engine.set_missing_list`): their imputing EM passes walk the list of the
    missing entries instead of the whole array."""
    prec = capi.precision_id(precision)                # an unknown string fails before the engine is touched
    # a dict is what dense_weight_blocks returned to the caller already: not checked and copied a second time
    dense_w = dense_entry_weights if isinstance(dense_entry_weights, dict) else dense_weight_blocks(Z, dense_entry_weights)
    listed = missing_list_blocks(Z, missing_list, dense_w, eng.comm_rank()[1] if missing_list else 1)
    observed = observed_only_blocks(Z, observed_only, sparse_sharding)
    weighted = entry_weight_blocks(Z, entry_weights, unstored_weight, observed, sparse_sharding)
    observed = sorted(set(observed) | set(weighted))
    lib = eng.lib
    nb_modes = len(Z['size'])
    which_p = _which_p(Z)
    P = len(Z['object'])
    lin = [int(v) for v in Z['coupling']['lin_coupled_modes']]
    nb_couplings = max(lin) if lin else 0
    if nb_couplings != len(Z['coupling']['coupling_type']):
        raise ValueError('Mismatch between number of coulings and coupling types')   # check_data_input.m:17-19
    for p in range(P):
        if Z['loss_function'][p] != 'Frobenius':
            raise capi.UnsupportedOnDevice(capi.ERR_UNSUPPORTED,
                                           "loss '%s' needs the L-BFGS-B path of the MATLAB code" % Z['loss_function'][p])
    miss = Z.get('miss') if Z.get('miss') is not None else [None] * P
    eng._resident_model = None
    capi.check(lib.aoadmm_model_begin(eng.h, nb_modes, P, nb_couplings))
    R_of = {}
    for p in range(P):
        md = [m - 1 for m in Z['modes'][p]]
        for m in md:
            R_of[m] = None
    # ranks come from the initial factors when given; here from the caller via Z['_ranks']
    ranks = Z['_ranks']
    for m in range(nb_modes):
        p = which_p[m]
        md = [q - 1 for q in Z['modes'][p]]
        if Z['model'][p] == 'PAR2' and md.index(m) == 1:
            rows = (C.c_int64 * len(Z['size'][m]))(*[int(v) for v in Z['size'][m]])
            capi.check(lib.aoadmm_model_set_mode_slabs(eng.h, m, len(Z['size'][m]), rows, int(ranks[m])))
        else:
            capi.check(lib.aoadmm_model_set_mode(eng.h, m, int(Z['size'][m]), int(ranks[m])))
    for p in range(P):
        md = [m - 1 for m in Z['modes'][p]]
        arr = (C.c_int * len(md))(*md)
        if Z['model'][p] == 'CP':
            capi.check(lib.aoadmm_model_add_cp(eng.h, p, len(md), arr, float(Z['weights'][p])))
        elif Z['model'][p] == 'PAR2':
            capi.check(lib.aoadmm_model_add_par2(eng.h, p, arr, float(Z['weights'][p])))
        else:
            raise ValueError("unknown model '%s'" % Z['model'][p])
    for m in range(nb_modes):
        if Z['constrained_modes'][m]:
            c = Z['constraints'][m]
            if c is None or len(c) == 0:
                raise ValueError('No constraint provided for mode %d.' % (m + 1))       # constraints_to_prox.m:10-12
            cid, params, Lmat = constraint_descriptor(c)
            capi.check(lib.aoadmm_model_set_constraint(eng.h, m, cid, capi.dptr(params) if params.size else None,
                                                       params.size, capi.dptr(Lmat) if Lmat is not None else None))
    ctm = Z['coupling'].get('coupl_trafo_matrices', [None] * nb_modes)
    ctm2 = Z['coupling'].get('coupl_trafo_matrices2', [None] * nb_modes)
    keep = []
    for m in range(nb_modes):
        H = capi.as_f(ctm[m]) if (lin[m] and ctm[m] is not None) else None
        H2 = capi.as_f(ctm2[m]) if (lin[m] and ctm2[m] is not None) else None
        keep += [H, H2]
        capi.check(lib.aoadmm_model_set_coupling(
            eng.h, m, lin[m] - 1, capi.dptr(H), H.shape[0] if H is not None else 0, H.shape[1] if H is not None else 0,
            capi.dptr(H2), H2.shape[0] if H2 is not None else 0, H2.shape[1] if H2 is not None else 0))
    for n in range(nb_couplings):
        capi.check(lib.aoadmm_model_set_coupling_type(eng.h, n, int(Z['coupling']['coupling_type'][n])))
    if Z.get('ridge') is not None:
        r = np.asarray(Z['ridge'], dtype=np.float64)
        capi.check(lib.aoadmm_model_set_ridge(eng.h, capi.dptr(r)))
    capi.check(lib.aoadmm_model_end(eng.h))
    model_prec = prec
    for p in range(P):
        if Z['model'][p] == 'CP':
            obj = Z['object'][p]
            # 'f16': dense 3-way blocks without a mask; matrices, order > 3 and masked blocks go up as fp32
            prec = model_prec
            if prec == capi.PREC_F16 and (len(Z['modes'][p]) != 3 or miss[p] is not None or p in dense_w):
                prec = capi.PREC_F32
            coo = None if isinstance(obj, dict) else coo_of(obj)
            if coo is not None:
                subs, vals, shape = coo
                md = [m - 1 for m in Z['modes'][p]]
                if tuple(shape) != tuple(int(Z['size'][m]) for m in md):
                    raise ValueError('Z.object{%d} has size %s, Z.size says %s' % (p + 1, tuple(shape), [Z['size'][m] for m in md]))
                if miss[p] is not None:                                              # cmtf_AOADMM.m:77-79
                    raise ValueError('Missing data (Z.miss) not supported for sptensor objects. Convert to tensor first.')
                if sparse_sharding:
                    eng.upload_coo(p, subs, vals, sharded=True)
                else:
                    eng.upload_coo(p, subs, vals)
                if p in observed:
                    if len(vals) == 0:
                        raise ValueError('sparse_observed_only: Z.object{%d} has no stored entry' % (p + 1))
                    eng.set_observed_only(p, True)
                if p in weighted:
                    w, alpha = weighted[p]
                    eng.set_entry_weights(p, None if w is None else subs, w, alpha)
                continue
            if isinstance(obj, dict) and obj.get('synthetic'):
                capi.check(lib.aoadmm_tensor_synth(eng.h, p, int(obj['rank']), int(obj['seed']), float(obj['noise']), prec))
            else:
                X = capi.as_f(obj)
                md = [m - 1 for m in Z['modes'][p]]
                if tuple(X.shape) != tuple(int(Z['size'][m]) for m in md):
                    raise ValueError('Z.object{%d} has size %s, Z.size says %s' % (p + 1, X.shape, [Z['size'][m] for m in md]))
                capi.check(lib.aoadmm_tensor_upload(eng.h, p, capi.dptr(X), prec))
            if p in dense_w:                                                         # carries Z.miss{p} as zeros
                eng.tensor_weights_upload(p, dense_w[p])
                continue
            if miss[p] is not None:                                                  # cmtf_AOADMM.m:78-97
                if isinstance(obj, dict):
                    raise ValueError('Z.miss needs explicit data in Z.object{%d}' % (p + 1))
                mk = np.asarray(miss[p])
                if tuple(mk.shape) != tuple(X.shape):
                    raise ValueError('Z.miss{%d} size does not match Z.object{%d}.' % (p + 1, p + 1))
                mk = np.asfortranarray(mk != 0, dtype=np.uint8)
                capi.check(lib.aoadmm_tensor_mask_upload(eng.h, p, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
                if p in listed:
                    eng.set_missing_list(p, True)
        elif _par2_sparse(Z['object'][p], p):
            # sparse slabs: the nonzeros of all slabs as (i, j, k) in one transfer; fp64 whatever `precision` says
            md = [m - 1 for m in Z['modes'][p]]
            Jk = [int(v) for v in Z['size'][md[1]]]
            if len(Z['object'][p]) != len(Jk):
                raise ValueError('Z.object{%d} has %d slabs, Z.size says %d' % (p + 1, len(Z['object'][p]), len(Jk)))
            subs, vals = pack_par2_slabs(Z['object'][p], int(Z['size'][md[0]]), Jk, p)
            if miss[p] is not None:
                raise ValueError('Missing data (Z.miss) not supported for sparse PARAFAC2 slabs. Convert to full slabs first.')
            eng.upload_par2_coo(p, subs, vals)
        else:
            # the slabs back to back (each I x J_k, column-major) in one transfer
            Xall = np.concatenate([np.asarray(Xk, dtype=np.float64).ravel(order='F') for Xk in Z['object'][p]])
            capi.check(lib.aoadmm_par2_slab_upload(eng.h, p, capi.ALL_SLABS, capi.dptr(Xall)))
            if miss[p] is not None:                                                  # :98-120
                K = len(Z['object'][p])
                if not isinstance(miss[p], (list, tuple)) or len(miss[p]) != K:
                    raise ValueError('Z.miss{%d} must be a cell array of length %d for PAR2.' % (p + 1, K))
                for k in range(K):
                    mk = np.asarray(miss[p][k])
                    if not np.all((mk == 0) | (mk == 1)):
                        raise ValueError('Z.miss{%d}{%d} must be a logical or binary (0/1) array.' % (p + 1, k + 1))
                    if tuple(mk.shape) != tuple(np.asarray(Z['object'][p][k]).shape):
                        raise ValueError('Z.miss{%d}{%d} size does not match Z.object{%d}{%d}.' % (p + 1, k + 1, p + 1, k + 1))
                    mk = np.asfortranarray(mk != 0, dtype=np.uint8)
                    capi.check(lib.aoadmm_par2_slab_mask_upload(eng.h, p, k, mk.ctypes.data_as(C.POINTER(C.c_uint8))))
    eng._resident_model = Z            # init_coupled_AOADMM_CMTF(nvecs = 1) on this Z takes its Gram matrices from here


def _put_cells(eng, field, index, cells):
    """A cell array of J_k x R matrices -> the device in one transfer (slab = AOADMM_ALL_SLABS)."""
    cells = [np.asarray(c, dtype=np.float64) for c in cells]
    cols = cells[0].shape[1]
    packed = np.concatenate([c.ravel(order='F') for c in cells])
    capi.check(eng.lib.aoadmm_state_set(eng.h, field, index, capi.ALL_SLABS, capi.dptr(packed),
                                        sum(c.shape[0] for c in cells), cols))


def _get_cells(eng, field, index, shapes):
    rows = sum(s[0] for s in shapes)
    cols = shapes[0][1]
    packed = np.zeros(rows * cols)
    capi.check(eng.lib.aoadmm_state_get(eng.h, field, index, capi.ALL_SLABS, capi.dptr(packed), rows, cols))
    out, o = [], 0
    for (r, c) in shapes:
        out.append(np.array(packed[o:o + r * c].reshape((r, c), order='F'), order='F'))
        o += r * c
    return out


def _put(eng, field, index, slab, a):
    a = capi.as_f(a)
    if a.ndim == 1:
        a = a.reshape(-1, 1, order='F')
    capi.check(eng.lib.aoadmm_state_set(eng.h, field, index, slab, capi.dptr(a), a.shape[0], a.shape[1]))


def _get(eng, field, index, slab, shape):
    out = np.zeros(shape, order='F')
    capi.check(eng.lib.aoadmm_state_get(eng.h, field, index, slab, capi.dptr(out), shape[0], shape[1]))
    return out


def upload_state(eng, Z, G):
    """The struct G -> device (init_coupled_AOADMM_CMTF.m:41-45)."""
    nb_modes = len(Z['size'])
    for m in range(nb_modes):
        F = G['fac'][m]
        if isinstance(F, (list, tuple)):
            _put_cells(eng, capi.F_FAC, m, F)
        else:
            _put(eng, capi.F_FAC, m, 0, F)
        for field, key in ((capi.F_CONSTRAINT_FAC, 'constraint_fac'), (capi.F_CONSTRAINT_DUAL, 'constraint_dual_fac'),
                           (capi.F_COUPLING_DUAL, 'coupling_dual_fac')):
            v = G.get(key, [None] * nb_modes)[m]
            if v is None or (isinstance(v, (list, tuple)) and len(v) == 0):
                continue
            if isinstance(v, (list, tuple)):
                _put_cells(eng, field, m, v)
            else:
                _put(eng, field, m, 0, v)
    for n, D in enumerate(G.get('coupling_fac', [])):
        if D is not None:
            _put(eng, capi.F_COUPLING_FAC, n, 0, D)
    for p, DB in G.get('DeltaB', {}).items():
        _put(eng, capi.F_DELTAB, p, 0, DB)
        _put_cells(eng, capi.F_P, p, G['P'][p])
        _put_cells(eng, capi.F_MU_DELTAB, p, G['mu_DeltaB'][p])


def download_state(eng, Z, G):
    """Device -> a struct with the same fields as G (the `Fac` output, cmtf_AOADMM.m:193)."""
    nb_modes = len(Z['size'])
    out = {k: (list(v) if isinstance(v, list) else dict(v) if isinstance(v, dict) else v) for k, v in G.items()}

    def pull(field, index, ref):
        if isinstance(ref, (list, tuple)):
            return _get_cells(eng, field, index, [np.shape(rk) for rk in ref])
        ref = np.asarray(ref)
        shp = ref.shape if ref.ndim == 2 else (ref.shape[0], 1)
        return _get(eng, field, index, 0, shp)

    for m in range(nb_modes):
        out['fac'][m] = pull(capi.F_FAC, m, G['fac'][m])
        for field, key in ((capi.F_CONSTRAINT_FAC, 'constraint_fac'), (capi.F_CONSTRAINT_DUAL, 'constraint_dual_fac'),
                           (capi.F_COUPLING_DUAL, 'coupling_dual_fac')):
            v = G.get(key, [None] * nb_modes)[m]
            if v is None or (isinstance(v, (list, tuple)) and len(v) == 0):
                continue
            out[key][m] = pull(field, m, v)
    for n, D in enumerate(G.get('coupling_fac', [])):
        if D is not None:
            out['coupling_fac'][n] = pull(capi.F_COUPLING_FAC, n, D)
    for p, DB in G.get('DeltaB', {}).items():
        out['DeltaB'][p] = pull(capi.F_DELTAB, p, DB)
        out['P'][p] = pull(capi.F_P, p, G['P'][p])
        out['mu_DeltaB'][p] = pull(capi.F_MU_DELTAB, p, G['mu_DeltaB'][p])
    return out


def _display_line(it, f, frm=None):
    """One row of the iteration table, format of cmtf_fun_AOADMM.m:55-58."""
    line = '%6d %12f %12f %12f %17f %12f' % (it, sum(f), f[0], f[1], f[2], f[3])
    return line + (' %12f' % frm if frm is not None else '')


def run_solver(eng, alg_options, nb_modes, has_missing=False):
    """`[Fac,out] = cmtf_fun_AOADMM(...)` (cmtf_AOADMM.m:193) -> the `out` struct (cmtf_fun_AOADMM.m:480-494)."""
    o = _make_options(alg_options)
    n = int(o.MaxOuterIters) + 1
    bufs = {k: np.zeros(n) for k in ('func_val_conv', 'func_coupl_conv', 'func_constr_conv', 'func_PAR2_coupl', 'time_at_it')}
    inner = np.zeros((nb_modes, max(int(o.MaxOuterIters), 1)), order='F')
    frm = np.full(n, np.nan)
    res = capi.Result()
    for k, b in bufs.items():
        setattr(res, k, capi.dptr(b))
    res.innerIters = capi.dptr(inner)
    res.func_rel_missing = capi.dptr(frm)
    # options.Display (cmtf_fun_AOADMM.m:44-59, :462-468, :498-504): 'iter' lines come live from inside the solve
    display = str(alg_options.get('Display', 'no')) if isinstance(alg_options, dict) else 'no'
    every = int(alg_options.get('DisplayIters', 10)) if isinstance(alg_options, dict) else 10
    rank0 = eng.comm_rank()[0] == 0
    cb = None
    if display in ('iter', 'final') and rank0:
        print(' Iter  f total      f tensors      f couplings    f constraints    f PAR2 couplings' +
              ('  f_rel_miss' if has_missing else ''))
        print('------ ------------ -------------  -------------- ---------------- ----------------')
    if display == 'iter' and rank0:
        def _line(_user, it, f, frm):
            print(_display_line(it, [f[i] for i in range(4)], frm if has_missing else None), flush=True)
        cb = capi.PROGRESS_FN(_line)
        capi.check(eng.lib.aoadmm_set_progress(eng.h, cb, None, every))
    try:
        capi.check(eng.lib.aoadmm_solve(eng.h, C.byref(o), C.byref(res)))
    finally:
        if cb is not None:
            capi.check(eng.lib.aoadmm_set_progress(eng.h, capi.PROGRESS_FN(0), None, 0))
    it = int(res.OuterIterations)
    if display in ('iter', 'final') and rank0:                                 # :496-503
        print('%6d %12f %12f %12f %12f %12f' % (it, res.f_tensors + res.f_couplings + res.f_constraints + res.f_PAR2_couplings,
                                                res.f_tensors, res.f_couplings, res.f_constraints, res.f_PAR2_couplings) +
              (' %12f' % res.f_rel_missing if has_missing else ''))
    out = {
        'f_tensors': res.f_tensors, 'f_couplings': res.f_couplings, 'f_constraints': res.f_constraints,
        'f_PAR2_couplings': res.f_PAR2_couplings, 'f_rel_missing': res.f_rel_missing,
        'OuterIterations': it,
        'innerIters': inner[:, :max(it, 1)].copy(),
    }
    for k, b in bufs.items():
        out[k] = b[:it + 1].copy()
    if has_missing:
        out['func_rel_missing'] = frm[:it + 1].copy()                          # cmtf_fun_AOADMM.m:490-492
    names = ['f_tensors', 'f_couplings', 'f_constraints', 'f_PAR2_couplings']
    if res.exit_code == 0:
        out['exit_flag'] = 'maxIterations'                                   # make_exit_flag.m:4-5
    elif res.exit_code == 2:
        out['exit_flag'] = 'heldoutPatience'                                 # alg_options.hip.heldout_patience
    elif res.exit_code == 3:
        out['exit_flag'] = 'rankPatience'                                    # alg_options.hip.rank_patience
    else:
        out['exit_flag'] = {nm: ('AbsFuncTol' if res.exit_abs[i] else 'RelFuncTol') for i, nm in enumerate(names)}
    return out


def cmtf_AOADMM(Z, alg_options=None, init='random', init_options=None, rng=None, engine=None, precision='f64'):
    """functions/cmtf_AOADMM.m:1-206.  Returns (Zhat, Fac, G, out)."""
    if alg_options is None:
        raise ValueError('alg_options are missing as input in cmtf_AOADMM.')
    eng = engine or default_engine()
    Z = dict(Z)
    which_p = _which_p(Z)
    for m, c in enumerate(Z['constraints']):                                          # cmtf_AOADMM.m:33-41
        if Z['constrained_modes'][m] and c is not None and c[0] == 'tPARAFAC2':
            p = which_p[m]
            if Z['model'][p] != 'PAR2' or [q - 1 for q in Z['modes'][p]].index(m) != 1:
                raise ValueError('The tPARAFAC2 constraint can only be impsed on the second mode of a PARAFAC2 model')
    if isinstance(init, dict):                                                        # :44-53
        G = init
    elif isinstance(init, str) and init.lower() == 'random':
        if init_options is None:
            raise ValueError('init_options are missing as input in cmtf_AOADMM.')
        G = init_coupled_AOADMM_CMTF(Z, init_options=init_options, rng=rng, engine=eng)
    else:
        raise ValueError('Initialization type not supported')
    nb_modes = len(Z['size'])
    ranks = []
    for m in range(nb_modes):
        F = G['fac'][m]
        ranks.append(int((F[0] if isinstance(F, (list, tuple)) else F).shape[1]))
    for p in range(len(Z['object'])):                                                 # :55-65
        if Z['model'][p] == 'PAR2':
            md = [q - 1 for q in Z['modes'][p]]
            for k, jk in enumerate(Z['size'][md[1]]):
                if jk < ranks[md[0]]:
                    raise ValueError('Number of components for PARAFAC2 is larger than size of slice %d of data tensor %d.' % (k + 1, p + 1))
    Z['_ranks'] = ranks
    # alg_options['hip']['sparse_sharding'] (default 0: replicated): sparse CP blocks sharded over the ranks
    hip = alg_options.get('hip', {}) if isinstance(alg_options, dict) else {}
    # alg_options['hip']['sparse_observed_only'] (default 0; 1: every sparse CP block; a list: 1-based block numbers):
    # the unstored entries of those blocks are missing, not zero
    sharding = bool(int(hip.get('sparse_sharding', 0)))
    observed_opt = hip.get('sparse_observed_only', 0)
    observed = observed_only_blocks(Z, observed_opt, sharding)
    # alg_options['hip']['sparse_entry_weights'] / ['sparse_unstored_weight'] (`entry_weight_blocks`): a weight in [0, 1]
    # per stored entry and one for the unstored entries of the named sparse CP blocks, which are observed-only as well
    weights_opt, alpha_opt = hip.get('sparse_entry_weights'), hip.get('sparse_unstored_weight')
    observed = sorted(set(observed) | set(entry_weight_blocks(Z, weights_opt, alpha_opt, observed, sharding)))
    # alg_options['hip']['entry_weights'] (`dense_weight_blocks`): an array of weights in [0, 1] per named DENSE CP block
    dense_w_opt = hip.get('entry_weights')
    dense_weighted = dense_weight_blocks(Z, dense_w_opt)
    # alg_options['hip']['missing_list'] (default 0; 1: every dense CP block with Z.miss; a list: 1-based block numbers):
    # the imputing EM passes of those blocks walk the list of their missing entries (`missing_list_blocks`)
    listed_opt = hip.get('missing_list', 0)
    missing_list_blocks(Z, listed_opt, dense_weighted, eng.comm_rank()[1] if listed_opt else 1)
    # alg_options['hip']['heldout'] = {1-based block: (subs, vals) | sptensor} and ['heldout_patience'] (`heldout_lists`):
    # entries kept out of the fit, scored on the device with every evaluation of the objective
    held = heldout_lists(Z, hip.get('heldout'), hip.get('heldout_patience', 0))
    # alg_options['hip']['rank_lists'] = {1-based block: dict(mode=, subs=, exclude=)} with ['rank_metric'], ['rank_every'],
    # ['rank_patience'] and ['rank_criterion'] (`rank_options`): ranking metrics of held-out rows tracked inside the solve
    rank = rank_options(Z, hip, hip.get('heldout_patience', 0))
    # alg_options['hip']['heldout_keep_best'] (default 0): 1 returns the iterate with the smallest held-out sum, or with
    # rank_criterion = 1 the one with the best ranking score
    keep_best = heldout_keep_best_option(hip.get('heldout_keep_best', 0), rank['lists'] if rank['criterion'] == 1 else held)
    build_model(eng, Z, precision, sparse_sharding=sharding, observed_only=observed_opt, entry_weights=weights_opt,
                unstored_weight=alpha_opt, dense_entry_weights=dense_weighted, missing_list=listed_opt)
    for p, (hs, hv) in sorted(held.items()):
        eng.set_heldout(p, hs, hv)
    for p, (rmode, rsubs, rexcl) in sorted(rank['lists'].items()):
        eng.set_ranklist(p, rmode, rsubs, exclude=rexcl)
    if rank['lists'] or rank['criterion']:
        eng.rank_track(rank['metric'], rank['k'], rank['every'], rank['patience'], rank['criterion'])
    if keep_best:
        eng.heldout_keep_best(True)
    upload_state(eng, Z, G)
    out = run_solver(eng, alg_options, nb_modes,
                     has_missing=bool(observed) or bool(dense_weighted) or (Z.get('miss') is not None and any(m is not None for m in Z['miss'])))
    if held:
        # out.func_heldout{block}: sum (y - m)^2 at iteration 0 .. OuterIterations; with heldout_sumsq = sum y^2 and
        # heldout_count the relative error sqrt(func_heldout / heldout_sumsq) and the RMSE sqrt(func_heldout /
        # heldout_count) follow.  The factors returned are those of the LAST iteration unless heldout_keep_best = 1
        out['func_heldout'], out['heldout_sumsq'], out['heldout_count'] = {}, {}, {}
        for p, (hs, hv) in sorted(held.items()):
            out['func_heldout'][p + 1], out['heldout_best_iter'] = eng.heldout_trace(p)
            out['heldout_sumsq'][p + 1] = float(np.sum(hv * hv))
            out['heldout_count'][p + 1] = int(hv.shape[0])
    if rank['lists']:
        # out.rank_trace{block}: per evaluation the iteration, the counts, the means hit / ndcg / mrr / auc and the raw sums
        # (`Engine.rank_trace`); out.rank_best_iter: the iteration of the best pooled score
        out['rank_trace'] = {p + 1: eng.rank_trace(p) for p in sorted(rank['lists'])}
        out['rank_best_iter'] = next(iter(out['rank_trace'].values()))['best_iter']
    if keep_best:
        # Fac and Zhat are the iterate heldout_best_iter (rank_criterion = 1: rank_best_iter); every other field of out still describes the whole run
        out['heldout_restored_iter'] = eng.heldout_restore_best()
    if int(hip.get('core_consistency', 0)):
        # alg_options['hip']['core_consistency'] = 1: out.core_consistency{0-based block} of every block the library can
        # project (3-way CP, not sharded, not observed-only), for the factors returned; the others are left out
        out['core_consistency'] = {}
        for p in range(len(Z['object'])):
            if Z['model'][p] != 'CP' or len(Z['modes'][p]) != 3:
                continue
            try:
                out['core_consistency'][p] = eng.core_consistency(p)
            except capi.UnsupportedOnDevice:
                pass
    Fac = download_state(eng, Z, G)
    Zhat = []
    for p in range(len(Z['object'])):                                                 # :197-206
        md = [q - 1 for q in Z['modes'][p]]
        if Z['model'][p] == 'CP':
            Zhat.append([Fac['fac'][m] for m in md])
        else:
            Zhat.append({'A': Fac['fac'][md[0]], 'Bk': Fac['fac'][md[1]], 'C': Fac['fac'][md[2]]})
    return Zhat, Fac, G, out
