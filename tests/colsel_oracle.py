"""Float64 NumPy restatements of LAESA.update_w (reference pymf/laesa.py:63-82) and of GMAP.update_w with robust_map=False
(pymf/gmap.py:119-165) for the tests.  H and ferr come from sivm_oracle.update_h: both classes inherit AA's H step.

  laesa_update_w  SIVM's start (sivm.py:145-166), then the running minimum of the distances and its argmax
  gmap_update_w   the norms, the first argmax, then iterval *= f(cosine) and its argmax

Both return (select, W); `scores` (a list) receives the score vector of every argmax that appends to select; f32_ops rounds
what the device forms in fp32 -- the distances (LAESA), the sums of squares, the column sums and the dots (GMAP) -- through
float32."""
import numpy as np

from sivm_oracle import distance, f32


def laesa_update_w(V, k, metric="l2", init="fastmap", scores=None, f32_ops=False):
    V = np.asarray(V, dtype=np.float64)

    def dist(idx):
        d = distance(V, idx, metric)
        return f32(d) if f32_ops else d

    if init == "fastmap":
        cur = 0
        for _ in range(3):
            d = dist(cur)
            cur = int(np.argmax(d))
        if scores is not None:
            scores.append(d.copy())
    elif init == "origin":
        cur = -1
    else:
        raise ValueError(init)
    select = [cur]
    distiter = dist(select[-1])
    for _ in range(k - 1):
        d = dist(select[-1])
        distiter = np.where(d < distiter, d, distiter)
        if scores is not None:
            scores.append(distiter.copy())
        select.append(int(np.argmax(distiter)))
    return select, V[:, select]                 # (a -1 entry is a Python index: the last column, laesa.py:79)


def gmap_update_w(V, k, method="pca", scores=None, f32_ops=False):
    V = np.asarray(V, dtype=np.float64)
    r = f32 if f32_ops else (lambda a: a)
    norm = np.sqrt(r(np.sum(V ** 2, axis=0)))
    if method in ("pca", "aa"):
        iterval = norm.copy()
    elif method == "nmf":
        iterval = 1.0 - r(np.sum(V, axis=0)) / (np.sqrt(V.shape[0]) * norm)
    else:
        raise ValueError(method)
    if scores is not None:
        scores.append(iterval.copy())
    select = [int(np.argmax(iterval))]
    for _ in range(1, k):
        c = r(np.dot(V[:, select[-1]], V)) / (norm * norm[select[-1]])
        if method == "pca":
            c = (1.0 - np.abs(c)) * norm
        elif method == "aa":
            c = ((c * -1.0 + 1.0) / 2.0) * norm
        else:
            c = 1.0 - np.abs(c)
        iterval = c * iterval
        if scores is not None:
            scores.append(iterval.copy())
        select.append(int(np.argmax(iterval)))
    return select, V[:, select]
