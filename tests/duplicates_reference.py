"""float64 / scipy reference of the near-duplicate groups (K14), and the inputs its tests share.

The contract is stated against s64 = the float64 dot product of the bf16 rows, with delta = 2 * d * 2^-24: a pair with
s64 >= tau + delta is an edge, one with s64 < tau - delta is none, in between either answer is right.  So every input here
comes with a threshold whose dead zone [tau - delta, tau + delta) holds no admissible pair (`dead_zone_pairs`), and the
reference below is then the only right answer for labels, degrees, counts and the edge set.
"""
import functools

import numpy as np
import torch

# (N, d) of the main cases; the widest gap of the pair similarities inside [0.62, 0.66] is >= 4 delta for seeds 1..3
SHAPES = [(203, 64), (331, 128), (515, 256), (515, 768), (643, 1024)]
WALK = 23       # rows per random walk
STEP = 1.2      # step length of a walk, in units of 1 / sqrt(d) per coordinate
WINDOW = (0.62, 0.66)


def delta(d):
    """worst-case error of an f32-accumulated dot product of d terms whose absolute products sum to <= 1, doubled (the MFMA's
    internal order is not specified)"""
    return 2.0 * d * 2.0 ** -24


def to_bf16(x):
    """float array -> (float32 array holding the bf16-rounded values, torch bf16 CPU tensor)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.to(torch.float32).numpy(), t


def walks(n, d, seed):
    """Random walks on the sphere, restarted from a fresh unit vector every WALK rows, rows permuted, rounded to bf16:
    neighbours along a walk are similar, rows a few steps apart are not, so a threshold cuts walks into pieces."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, d))
    v = None
    for i in range(n):
        if i % WALK == 0:
            v = rng.standard_normal(d)
        else:
            v = v + STEP * rng.standard_normal(d) / np.sqrt(d)
        v = v / np.linalg.norm(v)
        x[i] = v
    x = x[rng.permutation(n)]
    return to_bf16(x)


def widest_gap(S, lo=WINDOW[0], hi=WINDOW[1]):
    """(tau, gap): the midpoint and the width of the widest gap between consecutive pair similarities inside [lo, hi]
    (the window's ends count as values)"""
    iu = np.triu_indices(S.shape[0], 1)
    v = S[iu]
    v = np.sort(np.concatenate([v[(v >= lo) & (v <= hi)], [lo, hi]]))
    k = int(np.argmax(np.diff(v)))
    return float((v[k] + v[k + 1]) / 2), float(v[k + 1] - v[k])


def similarity(x32):
    x = np.asarray(x32, dtype=np.float64)
    return x @ x.T


def admissible(n, group=None):
    """bool [n, n]: i != j and, with group ids, group[i] != group[j]"""
    adm = ~np.eye(n, dtype=bool)
    if group is not None:
        g = np.asarray(group)
        adm &= g[:, None] != g[None, :]
    return adm


def dead_zone_pairs(S, adm, tau, dl):
    """number of admissible unordered pairs whose s64 lies in [tau - dl, tau + dl): must be 0 for a case to have one answer"""
    return int((np.triu(adm, 1) & (S >= tau - dl) & (S < tau + dl)).sum())


def reference(x32, tau, group=None, page_of=None, pages=0):
    """Everything K14 returns, from float64: dict of labels, degree, best_idx, best_sim, summary, edges (sorted [E, 2],
    i < j), page_pairs ([pages, pages] or None), plus S, adm and `ambiguous` (rows whose two best admissible similarities are
    within 2 delta: either partner is a right best_idx there)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    x32 = np.asarray(x32)
    n, d = x32.shape
    S = similarity(x32)
    adm = admissible(n, group)
    E = adm & (S >= tau)
    ncomp, comp = connected_components(csr_matrix(E), directed=False)
    smallest = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    labels = smallest[comp].astype(np.int32)
    degree = E.sum(1).astype(np.int32)
    Se = np.where(E, S, -np.inf)
    best_idx = np.where(degree > 0, np.argmax(Se, axis=1), -1).astype(np.int32)  # argmax: the lowest index among equal values
    best_sim = np.where(degree > 0, Se.max(axis=1, initial=-np.inf), 0.0)
    Sa = np.where(adm, S, -np.inf)
    top2 = -np.sort(-Sa, axis=1)[:, :2] if n > 1 else np.zeros((n, 2))
    ambiguous = (degree > 0) & (n > 2) & (top2[:, 0] - top2[:, -1] <= 2 * delta(d))
    sizes = np.bincount(labels, minlength=n)
    big = sizes[sizes >= 2]
    edges = np.argwhere(np.triu(E, 1)).astype(np.int32)
    summary = np.array([len(edges), len(big), big.sum() if len(big) else 0, big.max() if len(big) else 0], dtype=np.int64)
    pp = None
    if pages:
        pp = np.zeros((pages, pages), dtype=np.int32)
        p = np.asarray(page_of)
        for i, j in edges:
            a, b = p[i], p[j]
            if 0 <= a < pages and 0 <= b < pages:
                pp[a, b] += 1
                if a != b:
                    pp[b, a] += 1
    return {"labels": labels, "degree": degree, "best_idx": best_idx, "best_sim": best_sim, "summary": summary, "edges": edges,
            "page_pairs": pp, "S": S, "adm": adm, "ambiguous": ambiguous}


@functools.lru_cache(maxsize=None)
def case(n, d, seed=1, pages=0):
    """One main case, computed once and shared (treat it as read-only): rows, threshold, and the reference.  pages > 0: group ids
    and page ids drawn from that many pages (group == page), else no group."""
    x32, xb = walks(n, d, seed)
    S = similarity(x32)
    tau, gap = widest_gap(S)
    group = np.random.default_rng(1000 + seed).integers(0, pages, n).astype(np.int32) if pages else None
    ref = reference(x32, tau, group, group, pages)
    return {"n": n, "d": d, "x32": x32, "xb": xb, "tau": tau, "gap": gap, "group": group, "pages": pages, "ref": ref,
            "dead": dead_zone_pairs(ref["S"], ref["adm"], tau, delta(d))}
