"""Spectral clustering of the window embeddings on the device: the opt-in counterpart of ``diarization.SpectralCluster``.

The host class restates the reference step for step (tiny_audio/diarization.py:49-106): a dense float64 ``cosine_similarity``, an
``argpartition`` per row, a dense Laplacian and ``scipy.linalg.eigh`` of the whole [N, N] matrix -- O(N^2) memory and O(N^3) time, of
which only the ``max_num_spks + 1`` smallest eigenpairs are read.  ``DeviceSpectralCluster`` computes those pairs only:

  laplacian            ``ops.spk_affinity``: normalised rows, f32 cosine, the row-wise top-``keep`` cut by bisection, symmetrisation,
                       degrees -- W [N, N] and deg [N] stay on the device, the Laplacian L = diag(deg) - W is never formed;
  smallest_eigenpairs  block Lanczos on L with block width 16 and a seeded Gaussian start block.  One step is one streaming pass over
                       W (``ops.spk_laplacian_matmul``), classical Gram-Schmidt twice against the WHOLE basis (``spk_panel_gram`` /
                       ``spk_panel_update``) and a Cholesky-QR of the new block, whose 16 x 16 factor is taken on the host in float64
                       -- the step's one synchronisation.  The products L Q_j are kept, so the projected pencil H = V^T (L V),
                       M = V^T V is two Gram products; it goes to the host, is symmetrised and solved in float64 (M is the identity
                       up to the f32 rounding of the basis; solving the pencil instead of assuming it costs nothing at <= 1024^2).
                       The m smallest Ritz vectors V y and their residuals |L v - lambda v| are computed on the device, with a true
                       product L v.  From 24 blocks on, every 8 blocks, the iteration stops once the largest of the m residuals is at
                       most 1e-5 * 2 max(deg) (Gershgorin's bound on lambda_max); the basis is capped at min(1024, N / 2) columns.  A
                       block whose Cholesky factor fails or has a pivot below sqrt(2^-24) of its largest or of 2 max(deg) (what the f32
                       Gram product and the f32 projections resolve) means the Krylov space is exhausted: Rayleigh-Ritz runs on what
                       exists;
  __call__             the reference's eigengap rule on the Ritz values, then ``k_means`` on [N, k] on the host as before.

The device result is used only when it is trustworthy: the iteration converged, and the widest eigengap exceeds the second widest
by more than 4 times the largest residual -- a residual bounds the distance of its Ritz value to an eigenvalue, every gap is a
difference of two values, so no admissible perturbation can change the argmax.  Otherwise, and below ``min_rows`` rows, the host
``SpectralCluster`` runs; ``last_info`` says which path ran and why.  Nothing here is a default: ``SpeakerClusterer(device=None)`` keeps
the host path bit for bit.
"""
from __future__ import annotations

import time

import numpy as np

from .diarization import SpectralCluster

BLOCK = 16                       # Lanczos block width
FIRST_CHECK, CHECK_EVERY = 24, 8  # blocks before the first convergence check, blocks between checks
MAX_COLS = 1024                  # cap of the Krylov basis (TA_SPK_MAX_COLS)
RESIDUAL_TOL = 1e-5              # relative to 2 max(deg) >= lambda_max
GAP_SAFETY = 4.0                 # widest gap - second widest > GAP_SAFETY * largest residual
MAX_ROWS = 32768                 # TA_SPK_MAX_N
MIN_ROWS = 2048                  # default of ``min_rows``: below it the host eigh takes about a second and nothing is gained
PIVOT_FLOOR = 2.0 ** -12         # sqrt(2^-24): below it a Cholesky pivot of an f32 Gram matrix is rounding


def _ops():
    """The kernel wrappers; a function so that the import of torch and of the HIP library waits for the first device call."""
    from . import ops
    return ops


def choose_k(lambdas, residuals, min_num_spks: int, max_num_spks: int):
    """The reference's eigengap rule on the m smallest Ritz values, and whether residuals this large can change its answer.
    -> (k, trusted, widest gap, second widest gap)."""
    gaps = np.diff(np.asarray(lambdas, dtype=np.float64)[min_num_spks - 1:max_num_spks + 1])
    if gaps.size == 0:
        return min_num_spks, True, 0.0, 0.0
    at = int(np.argmax(gaps))
    first = float(gaps[at])
    second = float(np.max(np.delete(gaps, at))) if gaps.size > 1 else -np.inf
    worst = float(np.max(residuals)) if len(residuals) else 0.0
    return at + min_num_spks, bool(first - second > GAP_SAFETY * worst), first, second


class DeviceSpectralCluster(SpectralCluster):
    """``SpectralCluster`` with the affinity, the Laplacian and the eigenpairs computed on ``device``."""

    def __init__(self, min_num_spks: int = 1, max_num_spks: int = 15, pval: float = 0.06, device="cuda", min_rows: int | None = None,
                 seed: int = 0, max_blocks: int | None = None):
        """min_rows: None -- ``MIN_ROWS`` (2048).  max_blocks: a cap on the Lanczos blocks below the built-in one (tests)."""
        super().__init__(min_num_spks=min_num_spks, max_num_spks=max_num_spks, pval=pval)
        self.device, self.min_rows, self.seed, self.max_blocks = device, (MIN_ROWS if min_rows is None else min_rows), seed, max_blocks
        self.last_info: dict = {}

    # ------------------------------------------------------------------ the pieces
    def laplacian(self, embeddings):
        """embeddings [N, D] (numpy or tensor) -> (W f32 [N, N], deg f32 [N]) on the device; L = diag(deg) - W."""
        import torch
        ops = _ops()
        e = torch.from_numpy(np.array(embeddings, dtype=np.float32, order="C")) if not torch.is_tensor(embeddings) else embeddings.float()
        e = e.to(self.device).contiguous()
        n = e.shape[0]
        if n > MAX_ROWS:
            raise ValueError(f"speaker clustering on the device takes at most {MAX_ROWS} windows, got {n}")
        W, deg, _ = ops.spk_affinity(e, ops.spk_keep(n, self.pval))
        return W, deg

    def _cholesky_qr(self, Y, out, scale: float = 0.0) -> bool:
        """out = Y R^-1 with R^T R = Y^T Y; the factor in float64 on the host.  False: Y is rank deficient at f32 resolution -- a pivot
        below PIVOT_FLOOR of the largest one, or of ``scale`` (the bound on |L| for a block L Q minus its projections, which carries
        an absolute f32 error proportional to |L|, not to what is left of it)."""
        import scipy.linalg
        import torch
        ops = _ops()
        G = ops.spk_panel_gram(Y, Y).cpu().numpy().astype(np.float64)          # the step's synchronisation
        G = 0.5 * (G + G.T)
        if not np.isfinite(G).all():
            return False
        try:
            R = np.linalg.cholesky(G).T
        except np.linalg.LinAlgError:
            return False
        d = np.abs(np.diag(R))
        if not d.min() > PIVOT_FLOOR * max(d.max(), scale):
            return False
        Rinv = scipy.linalg.solve_triangular(R, np.eye(R.shape[0]), lower=False)
        ops.spk_panel_combine(Y, torch.from_numpy(np.ascontiguousarray(Rinv, dtype=np.float32)).to(Y.device), out=out)
        return True

    def _ritz(self, W, deg, V, LV, c: int, m: int):
        """Rayleigh-Ritz on the first c columns -> (lambda [m] float64, vecs f32 [N, m] on the device, residual norms [m]); None
        when the projected pencil cannot be solved."""
        import scipy.linalg
        import torch
        ops = _ops()
        Vc, LVc = V[:, :c], LV[:, :c]
        H = ops.spk_panel_gram(Vc, LVc).cpu().numpy().astype(np.float64)
        M = ops.spk_panel_gram(Vc, Vc).cpu().numpy().astype(np.float64)
        H, M = 0.5 * (H + H.T), 0.5 * (M + M.T)
        if not (np.isfinite(H).all() and np.isfinite(M).all()):
            return None
        try:
            lam, y = scipy.linalg.eigh(H, M, subset_by_index=[0, m - 1])
        except (np.linalg.LinAlgError, ValueError):
            return None
        dev = V.device
        vecs = ops.spk_panel_combine(Vc, torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev))
        R = ops.spk_laplacian_matmul(W, deg, vecs)                              # L v, a true product, not (L V) y
        ops.spk_panel_update(R, vecs, torch.from_numpy(np.diag(lam).astype(np.float32)).to(dev))
        res = np.sqrt(np.clip(np.diag(ops.spk_panel_gram(R, R).cpu().numpy().astype(np.float64)), 0.0, None))
        return lam, vecs, res

    def smallest_eigenpairs(self, W, deg, m: int):
        """The m smallest eigenpairs of L = diag(deg) - W -> (lambda [m] float64 ascending, vecs f32 [N, m] on the device, residual
        norms [m] float64, info).  info: blocks, columns, converged, exhausted, tol, max_residual, seconds in the steps and in Ritz."""
        import torch
        ops = _ops()
        N = W.shape[0]
        nb_max = max(1, min(MAX_COLS, N // 2) // BLOCK)
        if self.max_blocks is not None:
            nb_max = max(1, min(nb_max, int(self.max_blocks)))
        if not 1 <= m <= min(ops.SPK_MAX_P, nb_max * BLOCK):
            raise ValueError(f"{m} eigenpairs from a basis of {nb_max * BLOCK} columns (at most {ops.SPK_MAX_P})")
        dev = W.device
        V = torch.empty((N, nb_max * BLOCK), device=dev, dtype=torch.float32)
        LV = torch.empty_like(V)
        Y = torch.empty((N, BLOCK), device=dev, dtype=torch.float32)
        Y2 = torch.empty_like(Y)
        dmax = float(deg.max())
        tol = RESIDUAL_TOL * 2.0 * dmax
        info = dict(blocks=0, columns=0, converged=False, exhausted=False, tol=tol, max_residual=float("inf"), t_steps=0.0, t_ritz=0.0)
        start = torch.randn((N, BLOCK), generator=torch.Generator().manual_seed(int(self.seed)), dtype=torch.float32).to(dev)
        # the start block is orthonormalised twice: the second pass removes what the f32 Gram product of the first left
        if not (self._cholesky_qr(start, Y2) and self._cholesky_qr(Y2, V[:, :BLOCK])):
            info["exhausted"] = True
            return np.zeros(0), None, np.zeros(0), info
        nb, out = 1, None
        while True:
            t0 = time.perf_counter()
            c = nb * BLOCK
            ops.spk_laplacian_matmul(W, deg, V[:, c - BLOCK:c], out=LV[:, c - BLOCK:c])
            last = nb >= nb_max
            if not last and not (nb >= FIRST_CHECK and (nb - FIRST_CHECK) % CHECK_EVERY == 0):
                out = None
            else:
                t1 = time.perf_counter()
                out = self._ritz(W, deg, V, LV, c, m)
                info["t_ritz"] += time.perf_counter() - t1
                t0 += time.perf_counter() - t1
                if out is not None and float(out[2].max()) <= tol:
                    info["converged"] = True
            if info["converged"] or last:
                info["t_steps"] += time.perf_counter() - t0
                break
            Y.copy_(LV[:, c - BLOCK:c])
            for _ in range(2):                                                  # classical Gram-Schmidt, twice, against the whole basis
                ops.spk_panel_update(Y, V[:, :c], ops.spk_panel_gram(V[:, :c], Y))
            grown = self._cholesky_qr(Y, V[:, c:c + BLOCK], scale=2.0 * dmax)
            info["t_steps"] += time.perf_counter() - t0
            if not grown:
                info["exhausted"] = True
                break
            nb += 1
        info["blocks"], info["columns"] = nb, nb * BLOCK
        if out is None:                                                         # stopped by exhaustion between two checks
            t1 = time.perf_counter()
            out = self._ritz(W, deg, V, LV, nb * BLOCK, m)
            info["t_ritz"] += time.perf_counter() - t1
            if out is not None and float(out[2].max()) <= tol:
                info["converged"] = True
        if out is None:
            return np.zeros(0), None, np.zeros(0), info
        info["max_residual"] = float(out[2].max())
        return out[0], out[1], out[2], info

    # ------------------------------------------------------------------ SpectralCluster's call
    def _host(self, embeddings, oracle_num, reason: str, **extra):
        self.last_info = dict(path="host", reason=reason, **extra)
        return SpectralCluster.__call__(self, embeddings, oracle_num=oracle_num)

    def __call__(self, embeddings: np.ndarray, oracle_num: int | None = None) -> np.ndarray:
        n = embeddings.shape[0]
        if n > MAX_ROWS:
            raise ValueError(f"speaker clustering on the device takes at most {MAX_ROWS} windows, got {n}")
        m = self.max_num_spks + 1
        if n < max(self.min_rows, 6):
            return self._host(embeddings, oracle_num, f"N = {n} < min_rows = {self.min_rows}")
        if m > min(32, max(1, min(MAX_COLS, n // 2) // BLOCK) * BLOCK) or embeddings.shape[1] > 256:
            return self._host(embeddings, oracle_num, f"max_num_spks + 1 = {m} or D = {embeddings.shape[1]} outside the kernels' envelope")
        t0 = time.perf_counter()
        W, deg = self.laplacian(embeddings)
        lam, vecs, res, info = self.smallest_eigenpairs(W, deg, m)
        if not info["converged"]:
            why = "Krylov space exhausted" if info["exhausted"] else f"not converged in {info['blocks']} blocks"
            return self._host(embeddings, oracle_num, f"{why}: largest residual {info['max_residual']:.3g} > {info['tol']:.3g}", **info)
        if oracle_num is not None:
            k, trusted, first, second = int(oracle_num), True, 0.0, 0.0
        else:
            k, trusted, first, second = choose_k(lam, res, self.min_num_spks, self.max_num_spks)
        if not trusted:
            return self._host(embeddings, oracle_num, f"ambiguous eigengap: widest {first:.3g} - second {second:.3g} <= "
                              f"{GAP_SAFETY:g} x residual {info['max_residual']:.3g}", **info)
        emb = vecs[:, :k].double().cpu().numpy()
        self.last_info = dict(path="device", reason="converged, eigengap decided", k=k, gap=first, second_gap=second,
                              t_spectral=time.perf_counter() - t0, **info)
        return self.cluster_embs(emb, k)
