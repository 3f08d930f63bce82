"""Host: the float64 reference of tests/cluster_ref.py against the project's own ``SpectralCluster`` (which restates the reference), and
its numpy block Lanczos -- an f32 product, float64 elsewhere -- against ``eigh``.  This pins the algorithm independently of the kernels."""
import numpy as np
import pytest

from tests import cluster_ref as R
from tiny_audio_amd.diarization import SpectralCluster


def test_generator_plants_what_it_says():
    E, spk = R.embeddings(700, S=4, seed=1)
    a = 700 // 3
    assert E.dtype == np.float32 and np.array_equal(E[a], E[a + 5]) and spk[a] == spk[a + 5]
    n = np.linalg.norm(E.astype(np.float64), axis=1)
    assert n[350] == pytest.approx(1e3, rel=1e-5) and n[351] == pytest.approx(1e-3, rel=1e-5)
    assert np.allclose(np.delete(n, [350, 351]), 1.0, atol=1e-6) and (spk == 3).sum() == 7
    assert [R.keep_of(n) for n in (6, 257, 700, 1536)] == [6, 15, 42, 92]
    E6, _ = R.embeddings(6, seed=6)
    assert E6.shape == (6, R.D_EMB) and np.array_equal(E6[2], E6[5])


@pytest.mark.parametrize("N", R.SIZES)
def test_affinity_is_the_host_chain(N):
    """W and deg equal what SpectralCluster's get_sim_mat / p_pruning / symmetrisation / get_laplacian give, wherever the cut is not a
    tie (argpartition leaves ties unspecified); undecided entries stay under 2 % of N keep."""
    E, _ = R.embeddings(N, seed=N)
    keep = R.keep_of(N)
    r = R.affinity(E, keep)
    sc = SpectralCluster()
    pruned = sc.p_pruning(sc.get_sim_mat(E.astype(np.float64)))
    lap = sc.get_laplacian(0.5 * (pruned + pruned.T))
    ok = ~r.skip
    assert np.abs(R.dense_laplacian(r.W, r.deg) - lap)[ok].max() < 1e-12
    assert (r.kept.sum(1) == keep).all() and r.undecided.sum() <= 0.02 * N * keep
    assert np.array_equal(r.W, r.W.T) and (np.diag(r.W) == 0).all()
    if keep == N:
        assert not r.undecided.any()


def test_tie_rule_keeps_the_lowest_columns():
    E, at = R.tie_embeddings()
    r = R.affinity(E, 15)
    for row in at[:3]:
        assert np.array_equal(np.flatnonzero(r.kept[row]), at[:15])


def test_bounds_hold_for_an_f32_evaluation():
    """The product gate admits a plain float32 evaluation and refuses one dropped term."""
    N = 257
    E, _ = R.embeddings(N, seed=N)
    r = R.affinity(E, R.keep_of(N))
    W, deg = r.W.astype(np.float32), r.deg.astype(np.float32)
    X = R.panel_block(N, 16, seed=5)
    want, bound = R.laplacian_matmul(W, deg, X)
    got = (deg[:, None] * X - W @ X).astype(np.float64)
    assert (np.abs(got - want) <= bound).all() and (got[:, 1] == 0).all()
    j = int(np.flatnonzero(W[0])[0])
    assert abs(W[0, j] * X[j, 0]) > bound[0, 0]


@pytest.mark.parametrize("N,S,noise,seed", ((700, 4, 1.6, 1), (R.N_EIG, 5, 1.6, 11), (R.N_EIG, 3, 2.5, 12)))
def test_block_lanczos_reproduces_eigh(N, S, noise, seed):
    if N == R.N_EIG:
        c = R.eig_case({5: "5spk", 3: "3spk"}[S])
        E, ref, lam_ref, vec_ref = c.E, c.ref, c.lam, c.vecs
    else:
        E, _ = R.embeddings(N, S=S, noise=noise, seed=seed)
        ref = R.affinity(E, R.keep_of(N))
        lam_ref, vec_ref = np.linalg.eigh(R.dense_laplacian(ref.W, ref.deg))
    lam, vecs, res, blocks = R.block_lanczos(R.dense_laplacian(ref.W, ref.deg), 11)
    tol = 1e-5 * 2 * ref.deg.max()
    print(f"N {N}: {blocks} blocks, largest residual {res.max():.3e} (rule {tol:.3e}), largest |lambda - eigh| {np.abs(lam - lam_ref[:11]).max():.3e}")
    assert res.max() <= tol and (np.abs(lam - lam_ref[:11]) <= res + 1e-9).all()
    k = R.eigengap_k(lam, 2, 10)
    assert k == R.eigengap_k(lam_ref, 2, 10)
    sc = SpectralCluster(2, 10)
    np.random.seed(0)
    a = sc.cluster_embs(vecs[:, :k], k)
    np.random.seed(0)
    b = sc.cluster_embs(vec_ref[:, :k], k)
    assert R.same_partition(a, b)
