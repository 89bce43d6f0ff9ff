"""The Kmeans / Cmeans golden cases (tests/golden/gen_golden_cluster.py) and how their data is rebuilt."""
import numpy as np

from cluster_oracle import blobs
from conftest import load_golden

KMEANS_GOLDENS = ["kmeans_doc_2x3_k2", "kmeans_37x29_k5", "kmeans_37x29_k5_noerr", "kmeans_300x64_k6", "kmeans_500x200_k12"]
CMEANS_GOLDENS = ["cmeans_37x29_k5", "cmeans_300x64_k6", "cmeans_300x64_k6_userw"]


def load_case(name):
    g = load_golden(name)
    if "blob_seed" in g:
        m, n, nb = (int(x) for x in g["blob_shape"])
        g["V"] = blobs(m, n, nb, int(g["blob_seed"]))[0]
    return g


def onehot(assigned, k):
    H = np.zeros((k, len(assigned)))
    H[assigned, np.arange(len(assigned))] = 1.0
    return H
