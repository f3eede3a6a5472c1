"""numpy fp64 restatement of what a dense PARAFAC2 block runs outside the B_k loop, written from oracle/aoadmm.py line for
line (line numbers are those of functions/cmtf_fun_AOADMM.m), with the prox from oracle.prox:

  mode_a       :160-178   T1_k = X_k B_k, GB_k = B_k'B_k, A = sum_k T1_k D_k, C = sum_k D_k GB_k D_k
  c_systems    :219-231   a_k = w diag(A' X_k B_k) (+ bsum), C_k = A'A .* B_k'B_k, rho_k, B_k = w C_k (+ ridge, bsum)
  CLoop        :232-248 with ADMM_constrained_only on per-row systems :600-606 and update_constraint :1420-1429
  c_coupled    :260-267 / :305-312 (per-row systems), :282-297 (the (K R)-system; a diagonal H'H splits it into rows)
  objective    :1262-1264, :1355, :1337, :1279-1281

The matrix-free sums (Amt, Csys, a, res, q, regv) also exist accumulated in np.longdouble (`ld=True`): the second host
evaluation the GPU tests take their floor from.  tests/test_par2_modes_host.py proves these functions are the oracle's.
"""
import numpy as np
import scipy.linalg as sla

from oracle import aoadmm as OA
from oracle import prox as OP

LD = np.longdouble


def _f(x, ld):
    return np.asarray(x, dtype=LD if ld else np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# mode A
# ---------------------------------------------------------------------------------------------------------------------
def mode_a(X, B, C, ld=False):
    """:160-165; ld: products and sums in longdouble."""
    K, R = C.shape
    T1 = [_f(X[k], ld) @ _f(B[k], ld) for k in range(K)]
    GB = [_f(B[k], ld).T @ _f(B[k], ld) for k in range(K)]                       # G_transp_G{mB}{k}  (:216-218)
    return dict(T1=np.stack(T1), GB=np.stack(GB), **mode_a_sums(T1, GB, C, ld))


def mode_a_sums(T1, GB, C, ld=False):
    K, R = C.shape
    I = T1[0].shape[0]
    Amt = np.zeros((I, R), dtype=LD if ld else np.float64)
    Csys = np.zeros((R, R), dtype=LD if ld else np.float64)
    for k in range(K):
        if ld:
            c = _f(C[k], True)
            Amt = Amt + _f(T1[k], True) * c[None, :]
            Csys = Csys + c[:, None] * _f(GB[k], True) * c[None, :]
        else:
            Dk = np.diag(C[k, :])
            Amt = Amt + T1[k] @ Dk                                               # :163 (X_k B_k D_k)
            Csys = Csys + Dk @ GB[k] @ Dk                                        # :164
    return dict(Amt=Amt, Csys=Csys)


def mode_a_system(Amt, Csys, w):
    """:169-171: what the common system build receives."""
    R = Csys.shape[0]
    return dict(A=w * Amt, rho=float(np.trace(Csys) / R), B=w * Csys)


# ---------------------------------------------------------------------------------------------------------------------
# mode C
# ---------------------------------------------------------------------------------------------------------------------
def c_systems(X, A, B, C, w=1.0, ridge=0.0, bsum_half=0.0, GA=None, GB=None, ld=False):
    """:219-231 up to (not including) the rho terms.  Returns a (K x R), rho (K), Bk (list of R x R)."""
    K, R = C.shape
    GA = A.T @ A if GA is None else GA
    a = np.zeros((K, R), dtype=LD if ld else np.float64)
    rho = np.zeros(K)
    Bk = []
    for k in range(K):
        GBk = B[k].T @ B[k] if GB is None else GB[k]
        if ld:
            a[k] = w * np.sum(_f(A, True) * (_f(X[k], True) @ _f(B[k], True)), axis=0)
        else:
            a[k] = w * np.diag(A.T @ X[k] @ B[k])                                # :221
        Ck = GA * GBk                                                            # :222
        rho[k] = np.trace(Ck) / R                                                # :223
        Bs = w * Ck                                                              # :224
        if ridge:
            Bs = Bs + ridge * np.eye(R)                                          # :225-227
        if bsum_half:
            a[k] = a[k] + bsum_half * C[k, :]                                    # :231
            Bs = Bs + bsum_half * np.eye(R)
        Bk.append(Bs)
    return dict(a=a, rho=rho, Bk=Bk)


class CLoop:
    """The uncoupled C update behind c_systems (:232-248).  Unconstrained: C(k,:) = B_k \\ a_k (:236).  Constrained:
    L_k = chol(B_k + rho_k/2 I) and ADMM_constrained_only on the K row systems (:600-606), update_constraint with
    max(rho) (:1423-1424), residuals of eval_res_ADMM_constr (:1079-1096).  Iterates are computed once and kept, so runs
    with tolerances walk the same `while` over the same states.  solve = 'cho' (the oracle's cho_solve) or 'inv' (explicit
    inverse: the reordered host evaluation)."""

    def __init__(self, sys, con, C, Z, mu, solve='cho'):
        self.a, self.rho, self.con, self.solve = np.asarray(sys['a'], dtype=np.float64), sys['rho'], con, solve
        K, R = self.a.shape
        self.L, self.Bsys = [], []
        for k in range(K):
            Bs = sys['Bk'][k]
            if con is not None:
                Bs = Bs + self.rho[k] / 2 * np.eye(R)                            # :238
                self.L.append(OA._chol_lower(Bs))                                # :239
            else:
                self.L.append(np.linalg.cholesky(Bs))                            # what the device factors for :236
            self.Bsys.append(Bs)
        self.prox = OP.constraints_to_prox([1], [con], [K])[0][0] if con is not None else None
        self.states = [dict(C=C, Z=Z, mu=mu, res=(np.inf, np.inf), scale=None)]

    def _row(self, k, rhs):
        if self.solve == 'cho':
            return sla.cho_solve((self.L[k], True), rhs)
        return np.linalg.inv(self.Bsys[k]) @ rhs

    def single(self):
        K = self.a.shape[0]
        if self.solve == 'cho':
            return np.stack([np.linalg.solve(self.Bsys[k], self.a[k]) for k in range(K)])   # :236
        return np.stack([self._row(k, self.a[k]) for k in range(K)])

    def _step(self):
        s = self.states[-1]
        K, R = self.a.shape
        fac = np.zeros((K, R))
        for k in range(K):                                                       # :602-606
            A_inner = self.a[k] + self.rho[k] / 2 * (s['Z'][k, :] - s['mu'][k, :])
            fac[k, :] = self._row(k, A_inner)
        with np.errstate(invalid='ignore', divide='ignore'):
            Z = self.prox(fac + s['mu'], float(np.max(self.rho)))                # :1423-1424
            mu = s['mu'] + fac - Z                                               # :1428
            nf = OA._fro(fac)
            pr = OA._fro(fac - Z) / nf                                           # :1085
            scaling = OA._fro(mu)
            d = OA._fro(Z - s['Z'])
            du = d / scaling if scaling > 0 else d                               # :1087-1092
        # what each residual is a ratio of: the scale of its error bound (see tests/test_gpu_par2_bloop.py)
        scale = ((nf + OA._fro(Z)) / nf if nf > 0 else 0.0,
                 (OA._fro(s['Z']) + OA._fro(Z)) / (scaling if scaling > 0 else 1.0))
        self.states.append(dict(C=fac, Z=Z, mu=mu, res=(float(pr), float(du)), scale=scale))

    def run(self, max_inner, tol=(0.0, 0.0)):
        it, res = 0, (np.inf, np.inf)
        while it < max_inner and (res[0] > tol[0] or res[1] > tol[1]):           # :600
            it += 1
            if len(self.states) <= it:
                self._step()
            res = self.states[it]['res']
        out = dict(self.states[it])
        out['inner_iters'] = it
        return out

    def history(self, n):
        self.run(n)
        return [[s['res'][q] for s in self.states[1:n + 1]] for q in range(2)]


def c_coupled(sys, system, constrained, sysmat=None):
    """Systems of a C mode inside a coupling.  system 1: types 0, 3, 4 (:260-267); 2: type 2 with sysmat = H H'
    (:305-312); 3 / 4: types 1, 5 with H'H = diag(sysmat) / sysmat (:282-297, mean(rho) for the scalar rho).  Returns
    L (list; the raw B_k for system 4), M (system 4), rho_max / rho_mean / rho_sum."""
    rho, Bk = sys['rho'], sys['Bk']
    K, R = len(Bk), Bk[0].shape[0]
    con = 1 if constrained else 0
    out = dict(rho_max=float(np.max(rho)), rho_mean=float(np.mean(rho)), rho_sum=float(np.sum(rho)), M=None)
    rc = float(np.mean(rho))                                                     # :284
    if system in (1, 2):
        L = []
        for k in range(K):
            Bs = Bk[k]
            if system == 2:
                Bs = Bs + rho[k] / 2 * sysmat                                    # :307
            else:
                Bs = Bs + rho[k] / 2 * np.eye(R)                                 # :262
            if con:
                Bs = Bs + rho[k] / 2 * np.eye(R)                                 # :264
            L.append(OA._chol_lower(Bs))
        out['L'] = L
    else:
        HtH = np.diag(sysmat) if system == 3 else sysmat
        B2 = rc / 2 * np.kron(HtH, np.eye(R))                                    # :283-284 (kron(H,I)'kron(H,I) = kron(H'H, I))
        B2 = sla.block_diag(*Bk) + B2                                            # :286
        if con:
            B2 = B2 + rc / 2 * np.eye(K * R)                                     # :292
        if system == 3:
            # kron(diag(d), I) is block diagonal: the factor of B2 is the K factors of its diagonal blocks
            out['L'] = [np.linalg.cholesky(B2[k * R:(k + 1) * R, k * R:(k + 1) * R]) for k in range(K)]
            assert np.array_equal(B2, sla.block_diag(*[B2[k * R:(k + 1) * R, k * R:(k + 1) * R] for k in range(K)]))
        else:
            out['L'] = list(Bk)
            out['M'] = B2
    return out


# ---------------------------------------------------------------------------------------------------------------------
# objective pieces
# ---------------------------------------------------------------------------------------------------------------------
def reg_value(con, Bk, ld=False):
    """reg_func of constraints_to_prox for one slab (:1279-1281); ld: the same sums in longdouble."""
    if not ld:
        return float(OP.constraints_to_prox([1], [con], [[Bk.shape[0]]])[1][0](Bk))
    x, eta, name = _f(Bk, True), LD(con[1]), con[0]
    if name == 'l1 regularization':
        return eta * np.sum(np.abs(x))
    if name == 'l0 regularization':
        return eta * LD(np.count_nonzero(x))
    if name == 'l2 regularization':
        return eta * np.sum(np.sqrt(np.sum(x * x, axis=0)))
    if name == 'ridge':
        return eta * np.sum(x * x)
    if name == 'GL smoothness':
        return eta * np.sum((x[1:, :] - x[:-1, :]) ** 2)
    if name == 'TV regularization':
        return eta * np.sum(x[1:, :] - x[:-1, :])                                # the quirk of :81: no abs()
    raise ValueError(name)


def objective(X, A, B, C, P, DeltaB, Z=None, reg=None, ld=False):
    """res[k] = ||X_k - A D_k B_k'||_F^2 (:1262-1264); q[k] = ||B_k - P_k DeltaB||^2 (:1355), ||B_k||^2,
    ||B_k - Z_k||^2 (:1337; 0 without Z), ||B_k - B_{k-1}||^2 (t_smoothness_penalty; 0 for k = 0 and unequal sizes);
    regv[k] = reg_func(B_k) (:1279-1281)."""
    K = len(X)
    dt = LD if ld else np.float64
    res, q = np.zeros(K, dtype=dt), np.zeros((K, 4), dtype=dt)
    regv = np.zeros(K, dtype=dt) if reg is not None else None
    sq = (lambda M: np.sum(_f(M, True) ** 2)) if ld else (lambda M: OA._fro(M) ** 2)
    for k in range(K):
        if ld:
            Mk = (_f(A, True) * _f(C[k], True)[None, :]) @ _f(B[k], True).T
            res[k] = np.sum((_f(X[k], True) - Mk) ** 2)
            PD = _f(P[k], True) @ _f(DeltaB, True)
        else:
            Mk = A @ np.diag(C[k, :]) @ B[k].T                                   # :1262
            res[k] = OA._fro(X[k] - Mk) ** 2                                     # :1263
            PD = P[k] @ DeltaB
        q[k, 0] = sq(_f(B[k], ld) - PD)
        q[k, 1] = sq(B[k])
        if Z is not None:
            q[k, 2] = sq(_f(B[k], ld) - _f(Z[k], ld))
        if k > 0 and B[k].shape == B[k - 1].shape:
            q[k, 3] = sq(_f(B[k], ld) - _f(B[k - 1], ld))
        if reg is not None:
            regv[k] = reg_value(reg, B[k], ld)
    return dict(res=res, q=q, regv=regv)
