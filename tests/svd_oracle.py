"""Float64 NumPy restatement of pymf/svd.py (dense data) and pymf/pca.py, and its "float32 twin".

The oracle is the reference's arithmetic written out: the Gram matrix on the short side, eigh, the 1e-8 cut, descending
order, S = sqrt, the other side projected (svd.py:110-158); PCA centres, takes the leading columns of U and H = W^T data
(pca.py:73-108).  tests/test_svd_oracle_golden.py holds it to goldens made by the real reference.

The twin (f32=True) models the only float32 roundings of the device path: the data are rounded to float32 (the upload), the
Gram matrix and its eigenpairs stay float64 (k_prod_f64, Jacobi), and the projected side is a float32 product of float32
operands (U = data (v_i / s_i), or V = (u_i / s_i)^T data), as are PCA's H = W^T data and its float32 W.  The deviation between
oracle and twin is what the device tolerances are derived from (tests/svd_cases.py).
"""
import numpy as np

EPS = 1e-8            # svd.py:74


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _mm32(a, b):
    return np.dot(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)).astype(np.float64)


def gram_eig(data):
    """(left, kept eigenvalues descending, their eigenvectors as columns, all eigenvalues) of the Gram matrix on the short side."""
    rows, cols = data.shape
    left = rows > cols
    AA = np.dot(data.T, data) if left else np.dot(data, data.T)
    values, vectors = np.linalg.eigh(AA)
    keep = values > EPS
    vectors, kept = vectors[:, keep], values[keep]
    idx = np.argsort(kept)[::-1]
    return left, kept[idx], vectors[:, idx], values


def svd(data, f32_twin=False):
    """U (rows x r), S (r x r), V (r x cols) as svd.py:110-158 computes them."""
    data = f32(data) if f32_twin else np.asarray(data, dtype=np.float64)
    left, values, vectors, _ = gram_eig(data)
    s = np.sqrt(values)
    if left:                                                   # svd.py:136-158
        V = vectors.T
        U = _mm32(data, vectors / s) if f32_twin else np.dot(np.dot(data, vectors), np.diag(1.0 / s))
    else:                                                      # svd.py:111-133
        U = vectors
        V = _mm32((vectors / s).T, data) if f32_twin else np.dot(np.diag(1.0 / s), np.dot(U.T, data))
    return U, np.diag(s), V


def svd_ferr(data, U, S, V):                                   # svd.py:92-107
    return float(np.sqrt(np.sum((np.asarray(data, dtype=np.float64) - np.dot(np.dot(U, S), V)) ** 2)))


def centre(data, center_mean=True):                            # pca.py:73-82
    if not center_mean:
        return data
    return data - data[:, :].mean(axis=1).reshape(data.shape[0], -1)


def pca(data, num_bases=0, center_mean=True, f32_twin=False):
    """dict(W, H, eigenvalues, ferr, data) of one PCA.factorize() (pca.py:90-108, nmf.py:100-114); `data` is the centred array."""
    cd = centre(np.asarray(data), center_mean)
    cd = f32(cd) if f32_twin else np.asarray(cd, dtype=np.float64)
    U, S, _ = svd(cd, f32_twin)
    s = np.diag(S)
    order = np.argsort(s)[::-1]
    if num_bases > 0:
        order = order[:num_bases]
    W = U[:, order]
    if f32_twin:
        W32 = f32(W)
        H = _mm32(W32.T, cd)
        ferr = float(np.sqrt(np.sum((cd - np.dot(W32, H)) ** 2)))
    else:
        H = np.dot(W.T, cd)
        ferr = float(np.sqrt(np.sum((cd - np.dot(W, H)) ** 2)))
    return dict(W=W, H=H, eigenvalues=s[order], ferr=ferr, data=cd)


def fix_signs(E, P, axis):
    """The sign of a singular pair is free: make the largest-magnitude entry of every vector of the eigenvector side E positive
    and flip the projected side P with it.  axis = 0: the vectors are columns of E and rows of P; 1: rows of E, columns of P."""
    E, P = np.array(E, dtype=np.float64), (None if P is None else np.array(P, dtype=np.float64))
    vec = E if axis == 0 else E.T
    sg = np.ones(vec.shape[1])
    for i in range(vec.shape[1]):
        if vec[np.argmax(np.abs(vec[:, i])), i] < 0:
            sg[i] = -1.0
    if axis == 0:
        return E * sg, (None if P is None else P * sg[:, None])
    return E * sg[:, None], (None if P is None else P * sg)


def fix_svd_signs(U, V, left):
    """(U, V) with the signs fixed on the eigenvector side (V for rows > cols, else U)."""
    if left:
        V2, U2 = fix_signs(V, U, 1)
        return U2, V2
    return fix_signs(U, V, 0)
