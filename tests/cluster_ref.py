"""CPU float64 reference of the speaker-clustering kernels (csrc/cluster.hip) and of the block Lanczos iteration that
tiny_audio_amd/spectral.py drives over them, the input generator, and the gates.  A plain module (no fixtures):
``tests/test_cluster_ref.py`` checks it on the host, ``tests/test_gpu_cluster.py`` compares the library with it,
``tests/test_cluster_host.py`` uses ``CpuOps`` to run the driver without a GPU.  The metric helpers are those of tests/rowwise_ref.py,
imported, not copied.

Gates -- all derived, none read off a kernel's output.  u = 2^-24; gamma(n) = n u / (1 - n u) bounds the error of ANY order of n f32
additions of exactly representable terms, relative to the sum of their magnitudes (Higham 4.4, as in tests/gemm_ref.py).
  affinity   |S_dev - S_64| <= t = (2 D + 4) u: each normalised row carries (D / 2 + 2) u (a D-term sum of squares, a square root, a
             division), the D-term dot product of two unit vectors D u.  A keep / drop decision of the row-wise cut is DECIDED when the
             f64 value is more than 2 t away from the other side of the row's threshold (``affinity``: a kept entry above the
             (keep + 1)-th largest value by more than 2 t, a dropped one below the keep-th largest by more than 2 t).  Every entry of W
             both of whose decisions are decided must match within t, zeros exactly; the others are skipped, and the test first asserts
             that they are at most 2 % of N keep.
  products   |Y - Y_64| <= gamma(n + 1) (|deg| |X| + |W| |X|) row by row, on the device's own W and deg; the panel operations the same
             over the summed dimension.
  eigenpairs residuals recomputed in f64 from the device's W and deg; Weyl (a Ritz value lies within its residual of an eigenvalue);
             Davis-Kahan for the column space (``test_gpu_cluster.py``).

Inputs (``embeddings``): S speakers with centroids ~ N(0, I_192) normalised; a window is the centroid of a random speaker plus
``noise`` N(0, I) / sqrt(192), renormalised and rounded to f32.  Planted: rows a and a + 5 bitwise identical (in every other row their
two similarities tie exactly), one row scaled by 1e3 and one by 1e-3 (the normalisation must absorb both), and -- from 64 rows on --
a last speaker with only 7 windows.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.rowwise_ref import F64, _gen  # noqa: F401  (the metric's dtype and the seeded generator)

U = 2.0 ** -24
D_EMB = 192
PVAL = 0.06
SIZES = (6, 257, 700)                 # keep = 6 = N (nothing pruned); one past a tile edge, keep = 15; keep = 42
N_EIG = 1536                          # the eigensolver, with min_rows lowered to 1024
EIG_CASES = {"5spk": dict(S=5, noise=1.6, seed=11), "3spk": dict(S=3, noise=2.5, seed=12)}


def gamma(n):
    return n * U / (1.0 - n * U)


def keep_of(n, pval=PVAL):
    return max(1, int(max(pval, 6.0 / n) * n))


def embeddings(N, S=4, noise=1.6, seed=0, plant=True):
    """-> (E f32 [N, 192], speaker of every row)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((S, D_EMB))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    spk = rng.integers(0, S - 1 if (plant and N >= 64 and S > 1) else S, size=N)
    if plant and N >= 64 and S > 1:
        spk[rng.choice(N, size=7, replace=False)] = S - 1                    # a speaker with only 7 windows
    x = cent[spk] + noise * rng.standard_normal((N, D_EMB)) / np.sqrt(D_EMB)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    E = x.astype(np.float32)
    if plant:
        a = N // 3
        b = min(a + 5, N - 1)
        E[b], spk[b] = E[a], spk[a]
        E[N // 2] *= np.float32(1e3)
        E[N // 2 + 1] *= np.float32(1e-3)
    return E, spk


def affinity(E, keep):
    """float64 from the f32 bits of E -> S, P (pruned, ties lowest column first), W, deg, and ``skip``: the entries of W whose value
    hangs on an undecided keep / drop decision at t = (2 D + 4) u."""
    E = np.asarray(E, dtype=np.float64)
    N, D = E.shape
    nrm = np.linalg.norm(E, axis=1, keepdims=True)
    Eh = E / np.where(nrm > 0, nrm, 1.0)
    S = Eh @ Eh.T
    t = (2 * D + 4) * U
    order = np.argsort(-S, axis=1, kind="stable")                            # descending, ties lowest column first
    kept = np.zeros((N, N), dtype=bool)
    np.put_along_axis(kept, order[:, :keep], True, axis=1)
    srt = np.take_along_axis(S, order, axis=1)
    v_k = srt[:, keep - 1]
    v_next = srt[:, keep] if keep < N else np.full(N, -np.inf)
    undecided = np.where(kept, S <= (v_next + 2 * t)[:, None], S >= (v_k - 2 * t)[:, None])
    P = np.where(kept, S, 0.0)
    W = 0.5 * (P + P.T)
    np.fill_diagonal(W, 0.0)
    skip = undecided | undecided.T
    np.fill_diagonal(skip, False)                                            # the diagonal is 0 whatever was decided
    return SimpleNamespace(S=S, P=P, kept=kept, W=W, deg=W.sum(1), skip=skip, undecided=undecided, t=t, tight_rows=int((v_k - v_next <= 2 * t).sum()))


def tie_embeddings(N=257, copies=40, seed=3):
    """A tie AT the threshold: ``copies`` bitwise identical rows at the (sorted) positions ``at`` among N otherwise random unit rows.  In
    a copy's row the ``copies`` entries at ``at`` are the largest and equal, so with keep = 15 < copies exactly the 15 lowest columns
    of ``at`` survive; W[at[x], at[y]] = s / 2 * ([y < keep] + [x < keep]) off the diagonal, s their common value."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D_EMB))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    E = x.astype(np.float32)
    at = np.sort(rng.choice(N, size=copies, replace=False))
    E[at] = E[at[0]]
    return E, at


def laplacian_matmul(W, deg, X):
    """-> (Y_64, the row-wise bound gamma(N + 1) (|deg| |X| + |W| |X|))."""
    W, deg, X = (np.asarray(v, dtype=np.float64) for v in (W, deg, X))
    N = W.shape[0]
    return deg[:, None] * X - W @ X, gamma(N + 1) * (np.abs(deg)[:, None] * np.abs(X) + np.abs(W) @ np.abs(X))


def panel_block(N, p, seed):
    """X f32 [N, p]: N(0, 1) with a zero column (column 1 when there is one, else none) and the last column scaled by 1e3."""
    X = np.random.default_rng(seed).standard_normal((N, p)).astype(np.float32)
    if p > 2:
        X[:, 1] = 0.0
    if p > 1:
        X[:, -1] *= np.float32(1e3)
    return X


def dense_laplacian(W, deg):
    L = -np.asarray(W, dtype=np.float64)
    L[np.diag_indices_from(L)] += np.asarray(deg, dtype=np.float64)
    return L


def eigengap_k(lambdas, min_num_spks, max_num_spks):
    """The reference's rule (tiny_audio/diarization.py:99-104)."""
    return int(np.argmax(np.diff(lambdas[min_num_spks - 1:max_num_spks + 1]))) + min_num_spks


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(a) == len(b) and len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def block_lanczos(L, m, seed=0, block=16, first_check=24, check_every=8, max_cols=1024, tol_rel=1e-5):
    """The algorithm of tiny_audio_amd/spectral.py in numpy: the product L Q in f32, everything else in float64.
    -> (lambda [m], vecs [N, m], true float64 residuals [m], blocks)."""
    L64 = np.asarray(L, dtype=np.float64)
    L32 = L64.astype(np.float32)
    N = L64.shape[0]
    nb_max = max(1, min(max_cols, N // 2) // block)
    tol = tol_rel * 2.0 * float(np.diag(L64).max())
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((N, block)))[0]
    V, LV = [Q], []
    while True:
        LV.append((L32 @ V[-1].astype(np.float32)).astype(np.float64))
        nb = len(V)
        if nb >= nb_max or (nb >= first_check and (nb - first_check) % check_every == 0):
            Vc, LVc = np.hstack(V), np.hstack(LV)
            H = Vc.T @ LVc
            lam, y = np.linalg.eigh(0.5 * (H + H.T))
            vecs = Vc @ y[:, :m]
            res = np.linalg.norm(L64 @ vecs - vecs * lam[:m], axis=0)
            if res.max() <= tol or nb >= nb_max:
                return lam[:m], vecs, res, nb
        Y = LV[-1].copy()
        Vc = np.hstack(V)
        for _ in range(2):
            Y -= Vc @ (Vc.T @ Y)
        V.append(np.linalg.qr(Y)[0])


class CpuOps:
    """The five operations of tiny_audio_amd/ops.py that spectral.py calls, in torch CPU float32 (the affinity through the float64
    reference, rounded): what lets the driver's decisions be tested without a GPU.  Not a fallback of the package: tests only."""
    SPK_MAX_P = 32

    @staticmethod
    def spk_keep(n, pval):
        return keep_of(n, pval)

    @staticmethod
    def spk_affinity(E, keep, **_):
        r = affinity(E.numpy(), keep)
        return torch.from_numpy(r.W.astype(np.float32)), torch.from_numpy(r.deg.astype(np.float32)), None

    @staticmethod
    def spk_laplacian_matmul(W, deg, X, out=None):
        y = deg[:, None] * X - W @ X
        return y if out is None else out.copy_(y)

    @staticmethod
    def spk_panel_gram(A, B, out=None):
        return A.T @ B

    @staticmethod
    def spk_panel_update(B, A, C):
        return B.sub_(A @ C)

    @staticmethod
    def spk_panel_combine(V, Z, out=None):
        y = V @ Z
        return y if out is None else out.copy_(y)


@functools.lru_cache(maxsize=None)
def eig_case(name):
    """The N = 1536 cases: embeddings, the float64 affinity, eigh of the float64 Laplacian (computed once, shared, never changed)."""
    c = EIG_CASES[name]
    E, spk = embeddings(N_EIG, S=c["S"], noise=c["noise"], seed=c["seed"])
    ref = affinity(E, keep_of(N_EIG))
    lam, vecs = np.linalg.eigh(dense_laplacian(ref.W, ref.deg))
    for a in (E, spk, lam, vecs):
        a.setflags(write=False)
    return SimpleNamespace(E=E, spk=spk, ref=ref, lam=lam, vecs=vecs, S=c["S"])
