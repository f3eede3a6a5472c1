"""Reference of the objective evaluation (CMTF_AOADMM_func_eval, functions/cmtf_fun_AOADMM.m:1213-1363) for models of
unmasked dense CP blocks, from the definitions and in np.longdouble.  Shared by tests/test_objective_ref_host.py (which
pins it to the oracle) and tests/test_gpu_objective.py (which holds the device evaluation to it: csrc/solver_objective.hip,
reduce_batch in csrc/small.hip, reg_value in csrc/misc.hip, the coupling images of csrc/solver_coupled.hip).

evaluate(Z, G) takes the struct Z (`object`, `modes`, `size`, `weights`, `constraints`, `coupling`, optional `ridge`) and
a state G (`fac`, `constraint_fac`, `coupling_fac`) and returns an ObjectiveRef:

    f_tensors      sum_p w_p ||X_p - [[A_1..A_N]]||^2, the residual taken entry by entry over the full array (no
                   normsq - 2<mttkrp, fac> + <had, gram> shortcut)
                   + the regulariser values of constraints_to_prox.m:  l1 eta sum|x|, l0 eta nnz, l2 eta sum_r ||x_r||,
                   ridge eta ||x||^2, GL smoothness eta sum (x[i+1] - x[i])^2, TV eta sum (x[i+1] - x[i]) (no abs: the
                   reference's quirk, which the device copies), quadratic eta trace(x' L x) with L as given
                   + Z.ridge[n] ||fac_n||^2
    f_couplings    per coupling the sum over its modes of ||gap|| / ||den|| (types 0..5 as oracle/aoadmm.py func_eval),
                   mean over the non-zero couplings
    f_constraints  ||fac - Z|| / ||fac|| per constrained mode, mean over the non-zero entries

and, per term, the magnitude S the term was cancelled from (`terms`: name, value, S):
    a tensor term       w (||X||^2 + 2 |<X, M>| + ||M||^2)         (what the device's shortcut sums and subtracts)
    a regulariser value the sum of the absolute values of its summands, TV included
    a ratio             its numerator and denominator sums of squares, which have no cancellation of their own
bounds(rel) turns a relative bound `rel` on every sum into absolute bounds on the three returned pieces:
    f_tensors      rel * sum S
    a ratio        sqrt(a (1 + rel)) / sqrt(b (1 - rel)) - sqrt(a / b), plus 4 roundings (two square roots, the division
                   and this reference's own rounding to fp64); a mean of k ratios adds k more
"""
import math

import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
REG_NAMES = ('l1 regularization', 'l0 regularization', 'l2 regularization', 'ridge', 'GL smoothness', 'TV regularization',
             'quadratic regularization')


def _ld(a):
    return np.asarray(a, dtype=LD)


def _sumsq(a):
    a = _ld(a)
    return LD(np.sum(a * a))


def model(U):
    """sum_r prod_n U_n(i_n, r), longdouble, one rank-one term at a time."""
    U = [_ld(u) for u in U]
    N, R = len(U), U[0].shape[1]
    M = np.zeros(tuple(u.shape[0] for u in U), dtype=LD)
    for r in range(R):
        T = U[0][:, r]
        for n in range(1, N):
            T = T[..., None] * U[n][:, r]
        M += T
    return M


def reg_value(c, x):
    """(value, sum of the absolute summands) of the regulariser cell c at x, or None if c carries no value."""
    if c is None or c[0] not in REG_NAMES:
        return None
    x = _ld(x)
    eta = LD(c[1])
    name = c[0]
    if name == 'l1 regularization':
        t = np.abs(x)
    elif name == 'l0 regularization':
        t = (x != 0).astype(LD)
    elif name == 'l2 regularization':
        t = np.sqrt(np.sum(x * x, axis=0))
    elif name == 'ridge':
        t = x * x
    elif name == 'GL smoothness':
        t = (x[1:, :] - x[:-1, :]) ** 2
    elif name == 'TV regularization':
        t = x[1:, :] - x[:-1, :]
    else:                                                # eta * trace(x' L x) = eta * sum_ijr x_ir L_ij x_jr
        L = _ld(c[2])
        v = LD(np.sum(x * (L @ x)))
        mag = LD(np.sum(np.abs(x) * (np.abs(L) @ np.abs(x))))
        return eta * v, abs(eta) * mag
    return eta * LD(np.sum(t)), abs(eta) * LD(np.sum(np.abs(t)))


def coupling_images(ct, F, D, H, H2):
    """(image of the factor, image of Delta, denominator) of one coupled mode (oracle/aoadmm.py func_eval)."""
    F, D = _ld(F), _ld(D)
    H = None if H is None else _ld(H)
    if ct == 0:
        return F, D, F
    if ct == 1:
        return H @ F, D, H @ F
    if ct == 2:
        return F @ H, D, F @ H
    if ct == 3:
        return F, H @ D, F
    if ct == 4:
        return F, D @ H, F
    return H @ F, D @ _ld(H2), H @ F


class ObjectiveRef:
    def __init__(self):
        self.terms = []                 # (name, value, S) of every summand of f_tensors, longdouble
        self.coupling_ratios = []       # per coupling: [(a, b)] numerator and denominator sums of squares per member mode
        self.constraint_ratios = []     # (a, b) per constrained mode
        self.f_tensors = self.f_couplings = self.f_constraints = 0.0

    @property
    def f(self):
        return self.f_tensors, self.f_couplings, self.f_constraints

    @property
    def mag_tensors(self):
        return float(sum(t[2] for t in self.terms))

    def term(self, name):
        return [t for t in self.terms if t[0] == name]

    @staticmethod
    def _mean_of_ratio_sums(groups):
        """groups: per entry a list of (a, b); value sum sqrt(a/b) per entry, mean over the non-zero entries"""
        vals = [sum((np.sqrt(a) / np.sqrt(b) for a, b in g), LD(0)) for g in groups]
        tot = sum(vals, LD(0))
        nz = sum(1 for v in vals if v != 0)
        return tot / nz if tot > 0 else tot

    @staticmethod
    def _ratio_bound(groups, rel):
        up = math.sqrt((1.0 + rel) / (1.0 - rel))
        tot, nz, k = 0.0, 0, 0
        for g in groups:
            s = 0.0
            for a, b in g:
                q = float(np.sqrt(a) / np.sqrt(b))
                s += q * (up * (1.0 + 4 * U64) - 1.0)
                k += 1
            tot += s
            nz += 1 if any(a != 0 for a, _ in g) else 0
        if nz == 0:
            return 0.0
        val = float(ObjectiveRef._mean_of_ratio_sums(groups))
        return tot / nz + (k + 1) * U64 * val

    def bounds(self, rel):
        """absolute bounds on (f_tensors, f_couplings, f_constraints) when every sum is known to `rel` of its S"""
        return (rel * self.mag_tensors,
                self._ratio_bound(self.coupling_ratios, rel),
                self._ratio_bound([[ab] for ab in self.constraint_ratios], rel))


def evaluate(Z, G):
    ref = ObjectiveRef()
    nb_modes = len(Z['size'])
    P = len(Z['object'])
    for p in range(P):
        if Z['model'][p] != 'CP' or (Z.get('miss') is not None and Z['miss'][p] is not None):
            raise ValueError('objective_ref covers unmasked dense CP blocks only')
        md = [m - 1 for m in Z['modes'][p]]
        X = _ld(Z['object'][p])
        M = model([G['fac'][m] for m in md])
        w = LD(Z['weights'][p])
        d = X - M
        ref.terms.append(('tensor %d' % p, w * LD(np.sum(d * d)),
                          abs(w) * (LD(np.sum(X * X)) + 2 * abs(LD(np.sum(X * M))) + LD(np.sum(M * M)))))
    for n in range(nb_modes):
        if Z['constrained_modes'][n]:
            rv = reg_value(Z['constraints'][n], G['fac'][n])
            if rv is not None:
                ref.terms.append(('reg %d' % n, rv[0], rv[1]))
    if Z.get('ridge') is not None:
        for n in range(nb_modes):
            v = LD(Z['ridge'][n]) * _sumsq(G['fac'][n])
            ref.terms.append(('ridge %d' % n, v, abs(v)))
    ref.f_tensors = float(sum((t[1] for t in ref.terms), LD(0)))

    lin = [int(v) for v in Z['coupling']['lin_coupled_modes']]
    ctm = Z['coupling'].get('coupl_trafo_matrices', [None] * nb_modes)
    ctm2 = Z['coupling'].get('coupl_trafo_matrices2', [None] * nb_modes)
    for c in range(max(lin) if lin else 0):
        ct = int(Z['coupling']['coupling_type'][c])
        g = []
        for j in [i for i, v in enumerate(lin) if v == c + 1]:
            fi, di, den = coupling_images(ct, G['fac'][j], G['coupling_fac'][c], ctm[j], ctm2[j])
            g.append((_sumsq(fi - di), _sumsq(den)))
        ref.coupling_ratios.append(g)
    ref.f_couplings = float(ref._mean_of_ratio_sums(ref.coupling_ratios))

    for n in range(nb_modes):
        cf = G['constraint_fac'][n] if G.get('constraint_fac') is not None else None
        if cf is None:
            continue
        F = _ld(G['fac'][n])
        ref.constraint_ratios.append((_sumsq(F - _ld(cf)), _sumsq(F)))
    ref.f_constraints = float(ref._mean_of_ratio_sums([[ab] for ab in ref.constraint_ratios]))
    return ref
