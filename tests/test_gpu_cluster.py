"""-m gpu: the speaker-clustering kernels (csrc/cluster.hip) and the block Lanczos driver (tiny_audio_amd/spectral.py) against the
float64 reference and the derived gates of tests/cluster_ref.py.  Every output buffer is pre-filled with NaN and followed by guard
elements that must stay NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import cluster_ref as R
from tests.golden import ecapa_recipe as ER
from tiny_audio_amd import ops, spectral
from tiny_audio_amd.diarization import LocalSpeakerDiarizer, SpeakerClusterer, SpectralCluster

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def guarded(*shape):
    """-> (a NaN-filled contiguous tensor of ``shape``, the NaN guard behind it in the same allocation)."""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), float("nan"), device=DEV)
    return flat[:n].view(*shape), flat[n:]


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def device_affinity(N, padded):
    """The device's W, deg and kept counts for the generator's N rows; ``padded``: rows padded to 4 floats (the default output)."""
    E, _ = R.embeddings(N, seed=N)
    e = torch.from_numpy(E).to(DEV)
    keep = R.keep_of(N)
    if padded:
        W, deg, kept = ops.spk_affinity(e, keep, want_kept=True)
        guards = ()
    else:
        W, gw = guarded(N, N)
        deg, gd = guarded(N)
        W, deg, kept = ops.spk_affinity(e, keep, out=W, deg=deg, want_kept=True)
        guards = (gw, gd)
    torch.cuda.synchronize()
    return E, W, deg, kept, guards


@pytest.mark.parametrize("N", R.SIZES)
def test_affinity(N):
    E, W, deg, kept, guards = device_affinity(N, False)
    keep = R.keep_of(N)
    ref = R.affinity(E, keep)
    n_skip = int(ref.undecided.sum())
    print(f"N {N} keep {keep}: {ref.tight_rows} rows with a threshold tighter than 2 t, {n_skip} undecided entries of {N * keep}")
    assert n_skip <= 0.02 * N * keep
    for g in guards:
        assert torch.isnan(g).all()
    Wd, degd = W.cpu().numpy().astype(np.float64), deg.cpu().numpy().astype(np.float64)
    assert np.isfinite(Wd).all() and np.isfinite(degd).all()
    assert torch.equal(bits(W), bits(W.t())) and (torch.diagonal(W) == 0).all()
    assert (kept.cpu().numpy() == keep).all()
    ok = ~ref.skip
    err = np.abs(Wd - ref.W)
    print(f"  largest |W - W_64| on decided entries {err[ok].max():.3e} (gate {ref.t:.3e})")
    assert (err[ok] <= ref.t).all()
    assert (Wd[ok & (ref.W == 0)] == 0).all()
    assert (np.abs(degd - Wd.sum(1)) <= R.gamma(N) * np.abs(Wd).sum(1)).all()
    # the padded default layout gives the same bits
    _, Wp, degp, keptp, _ = device_affinity(N, True)
    assert torch.equal(bits(Wp), bits(W)) and torch.equal(bits(degp), bits(deg)) and torch.equal(keptp, kept)


def test_affinity_cosine_alone_is_symmetric_and_within_t():
    """Phase 1 on its own: S against float64 on every entry, S == S^T bitwise, the scaled rows absorbed."""
    N = 257
    E, _ = R.embeddings(N, seed=N)
    S, g = guarded(N, N)
    ops.spk_affinity(torch.from_numpy(E).to(DEV), R.keep_of(N), out=S, phases=1)
    ref = R.affinity(E, R.keep_of(N))
    assert torch.isnan(g).all() and torch.equal(bits(S), bits(S.t()))
    err = np.abs(S.cpu().numpy().astype(np.float64) - ref.S)
    print(f"largest |S - S_64| {err.max():.3e} (gate {ref.t:.3e})")
    assert (err <= ref.t).all()


def test_affinity_ties_at_the_threshold_keep_the_lowest_columns():
    E, at = R.tie_embeddings()
    N, keep = E.shape[0], R.keep_of(E.shape[0])
    assert keep == 15 < len(at)
    W, deg, kept = ops.spk_affinity(torch.from_numpy(E).to(DEV), keep, want_kept=True)
    assert (kept.cpu().numpy() == keep).all()
    sub = W.cpu().numpy()[np.ix_(at, at)]
    s = sub[0, 1]
    assert abs(float(s) - 1.0) <= (2 * R.D_EMB + 4) * R.U
    low = np.arange(len(at)) < keep
    want = np.float32(0.5) * (s * low[None, :].astype(np.float32) + s * low[:, None].astype(np.float32))
    np.fill_diagonal(want, 0.0)
    assert np.array_equal(sub.view(np.int32), want.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("padded", (True, False))
@pytest.mark.parametrize("p", (1, 16, 32))
@pytest.mark.parametrize("N", R.SIZES)
def test_laplacian_matmul(N, p, padded):
    _, W, deg, _, _ = device_affinity(N, padded)
    X = R.panel_block(N, p, seed=N + p)
    Y, g = guarded(N, p)
    ops.spk_laplacian_matmul(W, deg, torch.from_numpy(X).to(DEV), out=Y)
    want, bound = R.laplacian_matmul(W.cpu().numpy(), deg.cpu().numpy(), X)
    got = Y.cpu().numpy().astype(np.float64)
    assert torch.isnan(g).all() and np.isfinite(got).all()
    err = np.abs(got - want)
    print(f"N {N} p {p}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    if p > 2:
        assert (got[:, 1] == 0).all()                                         # the zero column


@pytest.mark.parametrize("N,a,b", ((257, 48, 16), (700, 48, 16), (1536, 80, 80), (700, 1, 1)))
def test_panel_operations(N, a, b):
    rng = np.random.default_rng(N + a)
    wide = rng.standard_normal((N, a + 16)).astype(np.float32)
    Bn = R.panel_block(N, b, seed=N)
    wide_d, B = torch.from_numpy(wide).to(DEV), torch.from_numpy(Bn).to(DEV)
    A = wide_d[:, :a]                                                          # a column slice: leading dimension a + 16
    A64, B64 = wide[:, :a].astype(np.float64), Bn.astype(np.float64)
    C, g = guarded(a, b)
    ops.spk_panel_gram(A, B, out=C)
    C2 = ops.spk_panel_gram(A, B)
    assert torch.isnan(g).all() and torch.equal(bits(C), bits(C2))             # two runs, the same bits
    err, bound = np.abs(C.cpu().numpy() - A64.T @ B64), R.gamma(N) * (np.abs(A64).T @ np.abs(B64))
    print(f"gram N {N} [{a} x {b}]: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    if b > ops.SPK_MAX_P:
        return
    Cn = C.cpu().numpy()
    U1 = ops.spk_panel_update(B.clone(), A, C)
    U2 = ops.spk_panel_update(B.clone(), A, C)
    assert torch.equal(bits(U1), bits(U2))
    want = B64 - A64 @ Cn.astype(np.float64)
    bound = R.gamma(a + 1) * (np.abs(B64) + np.abs(A64) @ np.abs(Cn.astype(np.float64)))
    assert (np.abs(U1.cpu().numpy() - want) <= bound).all()
    Y, gy = guarded(N, b)
    ops.spk_panel_combine(A, C, out=Y)
    assert torch.isnan(gy).all() and torch.equal(bits(Y), bits(ops.spk_panel_combine(A, C)))
    assert (np.abs(Y.cpu().numpy() - A64 @ Cn.astype(np.float64)) <= R.gamma(a) * (np.abs(A64) @ np.abs(Cn.astype(np.float64)))).all()


@functools.lru_cache(maxsize=None)
def device_eigenpairs(name):
    c = R.eig_case(name)
    d = spectral.DeviceSpectralCluster(min_num_spks=2, max_num_spks=10, device=DEV, min_rows=1024)
    W, deg = d.laplacian(c.E)
    lam, vecs, res, info = d.smallest_eigenpairs(W, deg, 11)
    L = R.dense_laplacian(W.cpu().numpy(), deg.cpu().numpy())
    return c, lam, vecs.cpu().numpy().astype(np.float64), res, info, L, np.linalg.eigh(L)


@pytest.mark.parametrize("name", tuple(R.EIG_CASES))
def test_eigenpairs(name):
    c, lam, vecs, res, info, L, (lam_ref, vec_ref) = device_eigenpairs(name)
    print(f"{name}: {info['blocks']} blocks, largest residual {res.max():.3e} (stopping rule {info['tol']:.3e}), "
          f"largest |lambda - eigh| {np.abs(lam - lam_ref[:11]).max():.3e}")
    assert info["converged"] and not info["exhausted"] and res.max() <= info["tol"]
    assert info["tol"] == pytest.approx(1e-5 * 2 * np.diag(L).max(), rel=1e-6)
    true = np.linalg.norm(L @ vecs - vecs * lam[None, :], axis=0)
    assert (np.abs(true - res) <= R.gamma(R.N_EIG) * np.abs(L).sum(0).max()).all()
    # Weyl, one to one in order: a Ritz value lies within its residual of an eigenvalue -- by the theorem for the float64 residual
    # (which the line above ties to the reported one); 1e-10 is what eigh itself leaves on a matrix of norm ~ 100
    assert (np.abs(lam - lam_ref[:11]) <= true + 1e-10).all()
    k, trusted, _, _ = spectral.choose_k(lam, res, 2, 10)
    k_ref = R.eigengap_k(c.lam, 2, 10)
    assert trusted and k == k_ref == R.eigengap_k(lam_ref, 2, 10)
    gap = lam_ref[k] - lam_ref[k - 1]
    q = np.linalg.qr(vecs[:, :k])[0]
    smin = np.linalg.svd(vec_ref[:, :k].T @ q, compute_uv=False).min()
    print(f"  k {k}, gap behind it {gap:.3f}, 1 - smallest singular value {1 - smin:.3e} (gate {(res.max() / gap) ** 2:.3e})")
    assert smin >= 1 - (res.max() / gap) ** 2


@pytest.mark.parametrize("name", tuple(R.EIG_CASES))
def test_clusterer_labels_equal_the_host_partition(name):
    c = R.eig_case(name)
    dev = SpeakerClusterer(device=DEV)
    dev._spectral_cluster = spectral.DeviceSpectralCluster(min_num_spks=2, max_num_spks=10, device=DEV, min_rows=1024)
    np.random.seed(0)                                                          # k_means draws its starts from numpy's global state
    got = dev(c.E.astype(np.float64))
    assert dev._spectral_cluster.last_info["path"] == "device", dev._spectral_cluster.last_info
    np.random.seed(0)
    want = SpeakerClusterer()(c.E.astype(np.float64))
    assert R.same_partition(got, want)
    assert isinstance(SpeakerClusterer()._get_spectral_cluster(), SpectralCluster) and SpeakerClusterer().device is None


class StubSpeakerModel:
    """``embed_windows`` that returns the generator's rows, one per window."""

    def __init__(self, E):
        self.E = E

    def embed_windows(self, buf, starts, lengths, window):
        assert len(starts) == len(self.E)
        return torch.from_numpy(self.E)


def _diarize_both(monkeypatch, audio, model, frames):
    """``diarize`` with the device clusterer and with the host one.  Voting breaks ties by speaker NUMBER, so the segment lists of two
    equal partitions may differ; the comparison is therefore: the window labels are the same partition, and the host's labels
    renamed to the device's names give exactly the device's segments.  -> (device segments, host segments, the clusterers' infos)."""
    seen, calls = [], []
    real_call = spectral.DeviceSpectralCluster.__call__
    monkeypatch.setattr(spectral.DeviceSpectralCluster, "__call__", lambda self, *a, **k: (real_call(self, *a, **k), seen.append(self.last_info))[0])
    real_post = LocalSpeakerDiarizer._postprocess_segments.__func__
    monkeypatch.setattr(LocalSpeakerDiarizer, "_postprocess_segments",
                        classmethod(lambda cls, *a: (calls.append(a), real_post(cls, *a))[1]))
    np.random.seed(0)
    on_dev = LocalSpeakerDiarizer.diarize(audio, speaker_model=model, speech_frames=frames, cluster_device=DEV)
    np.random.seed(0)
    host = LocalSpeakerDiarizer.diarize(audio, speaker_model=model, speech_frames=frames, cluster_device=None)
    assert len(seen) == 1 and len(calls) == 2 and on_dev and host
    (wins, lab_dev, dur, vad), (_, lab_host, _, _) = calls
    assert R.same_partition(lab_dev, lab_host)
    to_dev = dict(zip(lab_host.tolist(), lab_dev.tolist()))
    assert real_post(LocalSpeakerDiarizer, wins, np.array([to_dev[x] for x in lab_host.tolist()]), dur, vad) == on_dev
    return on_dev, host, seen


def test_diarize_with_cluster_device(monkeypatch):
    """The whole ``diarize`` with a stub speaker model: one segment that cuts into exactly the 1536 windows of the eigenpair case."""
    monkeypatch.setattr(spectral, "MIN_ROWS", 1024)
    c = R.eig_case("3spk")
    n_samples = 12000 + 2400 * (R.N_EIG - 1)
    audio = np.zeros(n_samples + 1, np.float32)
    frames = [True] * (n_samples // 256)
    _, _, seen = _diarize_both(monkeypatch, audio, StubSpeakerModel(c.E.copy()), frames)
    assert seen[0]["path"] == "device", seen


def test_diarize_end_to_end_with_the_device_ecapa(monkeypatch):
    """A short two-voice recording through ``EcapaTdnnMI355X.random_init`` and the device clusterer (``MIN_ROWS`` lowered so that
    its kernels run; with this few windows the basis is capped before it converges and the host finishes, as designed)."""
    from tiny_audio_amd import ecapa as E
    monkeypatch.setattr(spectral, "MIN_ROWS", 32)
    m = E.EcapaTdnnMI355X(E.EcapaConfig(**ER.GEOMS["a"]), device=DEV).random_init(0)
    audio = np.concatenate([ER._voice(48000, 1 + i, (110.0, 290.0)[i % 2], 0.03) for i in range(4)]).astype(np.float32)
    frames = [True] * (len(audio) // 256 - 1)
    _, _, seen = _diarize_both(monkeypatch, audio, m, frames)
    print(seen[0]["path"], "--", seen[0]["reason"])


def test_envelope():
    with pytest.raises(ValueError, match="32768"):
        spectral.DeviceSpectralCluster(device=DEV)(np.zeros((32769, 4), np.float32))
    e = torch.zeros(8, 4, device=DEV)
    with pytest.raises(Exception, match="bad argument"):
        ops.spk_affinity(e, 9)
