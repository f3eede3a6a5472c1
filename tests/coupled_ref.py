"""numpy fp64 restatement of the coupled ADMM inner loop (functions/cmtf_fun_AOADMM.m:625-1075, residuals :1099-1210 and
:1079-1096, systems :253-404) for CP modes, all six coupling types.  Shared by tests/test_coupled_ref_host.py (which pins
it to oracle.aoadmm on the CPU) and tests/test_gpu_coupled_loop.py (which compares the device loop with it).

A mode is a dict: A (rows x R, the weighted MTTKRP), C (R x R, Hadamard product of the other modes' Gram matrices),
w (the block's weight; 1 when absent, which is what the device entry offers: C then carries the weight), fac, muD, and
for a constrained mode Z, mu and prox (a handle prox(x, rho) of oracle.prox); H / H2 as the coupling type needs them.

Residual slots of a mode (squared Frobenius norms, the order the device keeps them in):
  0 |fac - Z|  1 |fac|  2 |mu|  3 |Z - Zold|  4 |Tf(C) - Sd(Delta)|  5 |mu_Delta|  6 |Sd(dDelta)|  7 |denominator|
"""
import numpy as np
import scipy.linalg as sla

from oracle import aoadmm as OA


class RefCoupled:
    """ADMM_coupled_case0..5 in numpy.  Iterates are computed once and kept, so that runs with tolerances walk the same
    `while` over the same states.  solve: 'reference' (the reference's own operations: triangular solves with chol,
    scipy's solve_sylvester, mldivide / mrdivide for Delta) or 'device' (the device's formulation: multiplication by
    the explicit inverse inv(L L'), the Sylvester solve in the eigenbases of H'H and of B, inv(AA) for Delta)."""

    def __init__(self, ctype, modes, Delta, solve='reference'):
        assert solve in ('reference', 'device')
        self.ctype, self.solve, self.n = ctype, solve, len(modes)
        self.m = modes
        self.con = [md.get('prox') is not None for md in modes]
        self.rho, self.L, self.Binv, self.B, self.B2, self.eig = [], [], [], [], [], []
        for md, con in zip(modes, self.con):
            C = np.asarray(md['C'], dtype=np.float64)
            R = C.shape[0]
            rho = float(np.trace(C) / R)                                          # :115
            B = float(md.get('w', 1.0)) * C                                       # :116
            L = Binv = B2 = eig = None
            if ctype in (0, 3, 4):
                B = B + rho / 2 * np.eye(R)                                       # :269, :336, :358
                if con:
                    B = B + rho / 2 * np.eye(R)
            elif ctype == 2:
                B = B + rho / 2 * (md['H'] @ md['H'].T)                            # :314
                if con:
                    B = B + rho / 2 * np.eye(R)
            else:                                                                 # :288-293, :377-382
                B2 = rho / 2 * (md['H'].T @ md['H'])
                if con:
                    B2 = B2 + rho / 2 * np.eye(B2.shape[0])
                if solve == 'device':
                    lam, U = np.linalg.eigh(md['H'].T @ md['H'])
                    w, V = np.linalg.eigh(B)
                    eig = (rho / 2 * lam + (rho / 2 if con else 0.0), U, w, V)
            if ctype not in (1, 5):
                L = OA._chol_lower(B)
                if solve == 'device':
                    Binv = np.linalg.inv(L @ L.T)
            self.rho.append(rho); self.L.append(L); self.Binv.append(Binv); self.B.append(B); self.B2.append(B2)
            self.eig.append(eig)
        st = dict(fac=[np.array(md['fac'], dtype=np.float64) for md in modes],
                  muD=[np.array(md['muD'], dtype=np.float64) for md in modes],
                  Z=[np.array(md['Z'], dtype=np.float64) if c else None for md, c in zip(modes, self.con)],
                  mu=[np.array(md['mu'], dtype=np.float64) if c else None for md, c in zip(modes, self.con)],
                  Zold=[None] * self.n, Delta=np.array(Delta, dtype=np.float64), DeltaOld=None,
                  res=(np.inf,) * 4, slots=None)
        self.states = [st]

    # ---- the coupling maps: Tf(C_m) = Sd_m(Delta)
    def _sd(self, j, D):
        t, md = self.ctype, self.m[j]
        return md['H'] @ D if t == 3 else D @ md['H'] if t == 4 else D @ md['H2'] if t == 5 else D

    def _tf(self, j, F):
        t, md = self.ctype, self.m[j]
        return md['H'] @ F if t in (1, 5) else F @ md['H'] if t == 2 else F

    def _tf_adj(self, j, Y):
        t, md = self.ctype, self.m[j]
        return md['H'].T @ Y if t in (1, 5) else Y @ md['H'].T if t == 2 else Y

    def _step(self):
        s = self.states[-1]
        t, n = self.ctype, self.n
        D = s['Delta']
        fac = []
        for j in range(n):                                                        # primal updates
            r2 = self.rho[j] / 2
            A_inner = self.m[j]['A'] + r2 * self._tf_adj(j, self._sd(j, D) - s['muD'][j])   # :647 :724 :790 :860 :925 :1012
            if self.con[j]:
                A_inner = A_inner + r2 * (s['Z'][j] - s['mu'][j])                  # :649
            if t in (1, 5):
                if self.solve == 'reference':
                    fac.append(sla.solve_sylvester(self.B2[j], self.B[j], A_inner))   # :728, :1016
                else:
                    beta, U, w, V = self.eig[j]
                    fac.append(U @ ((U.T @ A_inner @ V) / (beta[:, None] + w[None, :])) @ V.T)
            elif self.solve == 'reference':
                fac.append(OA._solve_llt_right(A_inner, self.L[j]))                # :651, :929
            else:
                fac.append(A_inner @ self.Binv[j])
        if t in (0, 1, 2):                                                        # :661-675, :737-749, :805-811
            newD = np.zeros_like(D)
            sum_rho = 0.0
            for j in range(n):
                newD = newD + self.rho[j] * (self._tf(j, fac[j]) + s['muD'][j])
                sum_rho = sum_rho + self.rho[j]
            newD = 1.0 / sum_rho * newD
        else:
            AA = BB = 0.0
            for j in range(n):
                md = self.m[j]
                if t == 3:                                                        # :875-885
                    AA = AA + self.rho[j] * (md['H'].T @ md['H'])
                    BB = BB + self.rho[j] * (md['H'].T @ (fac[j] + s['muD'][j]))
                elif t == 4:                                                      # :939-963
                    AA = AA + self.rho[j] * (md['H'] @ md['H'].T)
                    BB = BB + self.rho[j] * (fac[j] + s['muD'][j]) @ md['H'].T
                else:                                                             # :1026-1054, rhoC of the last mode (:1032)
                    rhoC = self.rho[n - 1]
                    AA = AA + rhoC * (md['H2'] @ md['H2'].T)
                    BB = BB + rhoC * (md['H'] @ fac[j] + s['muD'][j]) @ md['H2'].T
            if self.solve == 'reference':
                newD = np.linalg.solve(AA, BB) if t == 3 else OA._mrdivide(BB, AA)
            else:
                newD = np.linalg.inv(AA) @ BB if t == 3 else BB @ np.linalg.inv(AA)
        dD = newD - D
        muD, Z, mu, Zold = [], [], [], []
        slots = np.zeros((n, 8))
        with np.errstate(invalid='ignore', divide='ignore'):
            pc = dc = pz = dz = 0.0
            nz = 0
            for j in range(n):
                num = self._tf(j, fac[j]) - self._sd(j, newD)
                muD.append(s['muD'][j] + num)                                      # :679 and the same line of every case
                den = self._tf(j, fac[j]) if t in (1, 2) else fac[j]               # :1125, :1143; C elsewhere
                dd = self._sd(j, dD)
                slots[j, 4:] = [OA._fro(num) ** 2, OA._fro(muD[j]) ** 2, OA._fro(dd) ** 2, OA._fro(den) ** 2]
                pc += OA._fro(num) / OA._fro(den)
                sc = OA._fro(muD[j])
                dc += OA._fro(dd) / sc if sc > 0 else OA._fro(dd)
                slots[j, 1] = OA._fro(fac[j]) ** 2
                if self.con[j]:                                                   # update_constraint :1420-1429
                    Zn = self.m[j]['prox'](fac[j] + s['mu'][j], self.rho[j])
                    mun = s['mu'][j] + fac[j] - Zn
                    Zold.append(s['Z'][j]); Z.append(Zn); mu.append(mun)
                    slots[j, 0] = OA._fro(fac[j] - Zn) ** 2
                    slots[j, 2] = OA._fro(mun) ** 2
                    slots[j, 3] = OA._fro(Zn - s['Z'][j]) ** 2
                    pz += OA._fro(fac[j] - Zn) / OA._fro(fac[j])                   # :1085
                    sz = OA._fro(mun)
                    dz += OA._fro(Zn - s['Z'][j]) / sz if sz > 0 else OA._fro(Zn - s['Z'][j])   # :1087-1092
                    nz += 1
                else:
                    Zold.append(None); Z.append(None); mu.append(None)
            pc, dc = pc / n, dc / n
            if nz:
                pz, dz = pz / nz, dz / nz                                         # else 0 (:690-691)
        self.states.append(dict(fac=fac, muD=muD, Z=Z, mu=mu, Zold=Zold, Delta=newD, DeltaOld=D,
                                res=(float(pc), float(pz), float(dc), float(dz)), slots=slots))

    def run(self, max_inner, tol=(0.0, 0.0, 0.0, 0.0)):
        """-> the state the loop leaves (a dict, never to be modified) with inner_iters.  tol and res: primal coupling,
        primal constraint, dual coupling, dual constraint."""
        it, res = 0, (np.inf,) * 4
        while it < max_inner and any(r > t for r, t in zip(res, tol)):            # :633
            it += 1
            if len(self.states) <= it:
                self._step()
            res = self.states[it]['res']
        out = dict(self.states[it])
        out['inner_iters'] = it
        return out

    def history(self, max_inner):
        """The four residual series over max_inner iterations at tolerance 0: [pr_coupl, pr_constr, du_coupl, du_constr]."""
        self.run(max_inner)
        return [[s['res'][k] for s in self.states[1:max_inner + 1]] for k in range(4)]
