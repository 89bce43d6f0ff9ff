"""Float64 NumPy restatement of AA (reference pymf/aa.py) for the tests.

  hull_qp        the EXACT projection of w onto the convex hull of the columns of V, for any n (Wolfe's minimum-norm-point
                 algorithm on the points v_j - w); returns beta (>= 0, sum 1).  beta is unique only for affinely independent
                 columns, V beta always is
  update_w       AA.update_w (aa.py:113-134): W_hat = V pinv(H), every column projected onto the hull; (W, beta)
  update_h       AA.update_h (aa.py:93-111), through sivm_oracle
  device_rounds  the device's W step restated round by round: pricing g = R^T V, the admission test, the
                 affine minimiser on the corral, Wolfe's minor cycles; switches round V, R and g to float32
  w_hat_f32      W_hat from a float32 product V (inv(H H^T) H)^T (the right-hand sides of the device's W step)
  gap            beta^T g - min g with g = V^T (V beta - w): ||V beta - x*||^2 <= gap for the projection x*, whatever solver
                 produced beta
"""
import numpy as np

import sivm_oracle as so

AA_TAU = 2e-6            # admission: g_min < beta^T g - AA_TAU |R| max(|v_e|, |X|)      (pmf_aa.h)
AA_RHO = 1e-6            # a base whose residual is below AA_RHO max(|w|, |X|) is finished
AA_PIV = 1e-10           # affine independence: the entering column's pivot against its diagonal entry
AA_MAX_CORRAL = 128


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def pinv(H, eps=1e-8):
    """svd.py:27-45: the pseudo-inverse through the SVD, singular values above eps."""
    U, s, Vt = np.linalg.svd(np.asarray(H, dtype=np.float64), full_matrices=False)
    keep = s > eps
    return (Vt[keep].T / s[keep]).dot(U[:, keep].T)


def _affine_min(A, idx):
    """The minimiser of |sum a_j p_j|^2, sum a = 1, over the points idx whose Gram matrix is A: (11^T + P^T P) u = 1, a = u / sum u.
    Returns (a, last pivot of the Cholesky factor squared)."""
    M = A[np.ix_(idx, idx)] + 1.0
    L = np.linalg.cholesky(M)
    u = np.linalg.solve(L.T, np.linalg.solve(L, np.ones(len(idx))))
    return u / u.sum(), L[-1, -1] ** 2


def _minor_cycles(A, slots, lam, entering):
    """Wolfe's minor cycles on the corral `slots` (a list; `lam` a dict slot -> weight): back to the simplex along the line to the
    affine minimiser, dropping what reaches zero, until the minimiser is inside.  Returns (slots, lam, entering dropped)."""
    dropped_entering = False
    while True:
        a, _ = _affine_min(A, slots)
        if np.all(a > 0):
            return slots, dict(zip(slots, a)), dropped_entering
        cur = np.array([lam[s] for s in slots])
        blocking = np.flatnonzero(a <= 0)
        theta = min(1.0, max(0.0, float(np.min(cur[blocking] / (cur[blocking] - a[blocking])))))
        new = cur + theta * (a - cur)
        drop = [q for q in blocking if new[q] <= 1e-15 * max(1.0, new.max())]
        if not drop:
            drop = [int(blocking[np.argmin(new[blocking])])]
        keep = [q for q in range(len(slots)) if q not in drop]
        dropped_entering = dropped_entering or any(slots[q] == entering for q in drop)
        lam = {slots[q]: max(new[q], 0.0) for q in keep}
        slots = [slots[q] for q in keep]


def _project(V, w, f32_r=False, f32_g=False, tau=AA_TAU, rho=AA_RHO, piv=AA_PIV, cap=100000, exact=False):
    """(beta, rounds).  exact: no tolerances (tau = rho = 0): Wolfe's algorithm as published, for hull_qp."""
    m, n = V.shape
    if exact:
        tau = rho = 0.0
    A = {}                                         # Gram matrix of d_j = v_j - w over the columns met so far

    def gram(cols):
        D = V[:, cols] - w[:, None]
        return D.T.dot(D)

    X = np.zeros(m)
    R = f32(-w) if f32_r else -w
    corral, lam = [], {}
    rounds = 0
    while rounds < cap:
        rounds += 1
        g = R.dot(V)
        if f32_g:
            g = f32((R.astype(np.float32)).dot(V.astype(np.float32)))
        e = int(np.argmin(g))                      # (the lowest index among equals)
        if corral:
            RR, RX, XX, ww, vv = R.dot(R), R.dot(X), X.dot(X), w.dot(w), V[:, e].dot(V[:, e])
            if RR <= rho * rho * max(ww, XX):
                break
            if not (g[e] < RX - tau * np.sqrt(RR) * np.sqrt(max(vv, XX))):
                break
            if e in corral:
                break
        trial = corral + [e]
        G = gram(trial)
        try:
            _, p = _affine_min(G, list(range(len(trial))))
        except np.linalg.LinAlgError:              # (a pivot at or below zero: an exact twin of a corral column)
            p = 0.0
        if not (p > piv * (G[-1, -1] + 1.0)):      # affinely dependent on the corral: refused
            break
        lam[e] = 0.0
        slots, lam, gone = _minor_cycles(G, list(range(len(trial))), {q: lam[c] for q, c in enumerate(trial)}, len(trial) - 1)
        corral = [trial[q] for q in slots]
        lam = {trial[q]: lam[q] for q in slots}
        Xd = V[:, corral].dot(np.array([lam[c] for c in corral]))
        X = f32(Xd) if f32_r else Xd
        R = f32(Xd - w) if f32_r else Xd - w
        if gone:
            break
    beta = np.zeros(n)
    for c in corral:
        beta[c] = lam[c]
    return beta, rounds, len(corral)


def hull_qp(V, w):
    V = np.asarray(V, dtype=np.float64)
    return _project(V, np.asarray(w, dtype=np.float64), exact=True)[0]


def w_hat(V, H):
    return np.asarray(V, dtype=np.float64).dot(pinv(H))


def w_hat_f32(V, H):
    """W_hat as the device forms it: M^T = inv(H H^T) H in float64, rounded once to float32, then V M^T with float32 operands,
    accumulation and result."""
    V32, Hd = np.asarray(V, dtype=np.float32), np.asarray(H, dtype=np.float32).astype(np.float64)
    MT = np.linalg.solve(Hd.dot(Hd.T), Hd).astype(np.float32)
    return V32.dot(MT.T).astype(np.float64)


def update_w(V, H):
    """(W, beta, W_hat): aa.py:113-134 with the exact solver."""
    V = np.asarray(V, dtype=np.float64)
    Wh = w_hat(V, H)
    beta = np.stack([hull_qp(V, Wh[:, i]) for i in range(Wh.shape[1])], axis=0)
    return V.dot(beta.T), beta, Wh


def update_h(V, W):
    return so.update_h(np.asarray(V, dtype=np.float64), np.asarray(W, dtype=np.float64))


def device_rounds(V, Wh, f32_v=False, f32_r=False, f32_g=False):
    """The device's W step from W_hat: (W, beta, rounds of the whole step, largest corral).  A round is one pricing pass and
    one master step for every base, so the step takes as many as its slowest base (its last round finds it finished)."""
    V = f32(V) if f32_v else np.asarray(V, dtype=np.float64)
    Wh = f32(Wh) if f32_r else np.asarray(Wh, dtype=np.float64)
    betas, rounds, corral = [], 0, 0
    for i in range(Wh.shape[1]):
        b, r, s = _project(V, Wh[:, i], f32_r=f32_r, f32_g=f32_g)
        betas.append(b)
        rounds = max(rounds, r)
        corral = max(corral, s)
    beta = np.stack(betas, axis=0)
    W = V.dot(beta.T)
    return (f32(W) if f32_r else W), beta, rounds, corral


def gap(V, w, beta):
    V = np.asarray(V, dtype=np.float64)
    g = V.T.dot(V.dot(beta) - np.asarray(w, dtype=np.float64))
    return float(beta.dot(g) - g.min())
