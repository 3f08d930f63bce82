"""Host: the C ABI, the operators and the dry-run plumbing of the speaker-clustering kernels, and the decisions of
``DeviceSpectralCluster`` -- which path runs and what ``last_info`` says -- with the five operations emulated on the CPU
(``tests/cluster_ref.CpuOps``)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cluster_ref as R
from tiny_audio_amd import _lib, ops, spectral, torch_ops
from tiny_audio_amd.diarization import LocalSpeakerDiarizer, SpeakerClusterer, SpeakerDiarizer, SpectralCluster


@pytest.fixture
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


@pytest.fixture
def cpu_ops(monkeypatch):
    monkeypatch.setattr(spectral, "_ops", lambda: R.CpuOps)


# ----------------------------------------------------------------------------- header, library, operators
def test_header_declares_and_cites():
    text = open(_lib.HEADER).read()
    for cite in ("tiny_audio/diarization.py:49-106", "tiny_audio/diarization.py:49-86", "tiny_audio/diarization.py:87-89",
                 "tiny_audio/diarization.py:91-106", "#define TA_SPK_MAX_N 32768", "#define TA_SPK_MIN_N 6", "#define TA_SPK_MAX_D 256",
                 "#define TA_SPK_MAX_P 32", "#define TA_SPK_MAX_COLS 1024"):
        assert cite in text, cite
    protos = _lib.parse_header()
    for name, nargs in (("ta_spk_affinity_f32", 11), ("ta_spk_affinity_ws_floats", 2), ("ta_spk_laplacian_matmul_f32", 11),
                        ("ta_spk_lapmul_ws_floats", 2), ("ta_spk_panel_gram_f32", 11), ("ta_spk_gram_ws_floats", 3),
                        ("ta_spk_panel_update_f32", 10), ("ta_spk_panel_combine_f32", 10)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert "cluster.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    assert (ops.SPK_MIN_N, ops.SPK_MAX_N, ops.SPK_MAX_D, ops.SPK_MAX_P, ops.SPK_MAX_COLS) == (6, 32768, 256, 32, 1024)
    assert spectral.MAX_ROWS == ops.SPK_MAX_N and spectral.MAX_COLS == ops.SPK_MAX_COLS


def test_c_abi_sizes_and_refusals():
    """Host-only entry points and the argument checks that return before any launch."""
    L = _lib.lib()
    assert L.ta_spk_affinity_ws_floats(257, 192) == 257 * 192 and L.ta_spk_affinity_ws_floats(257, 190) == 257 * 192
    assert L.ta_spk_affinity_ws_floats(5, 192) == 0 and L.ta_spk_affinity_ws_floats(32769, 192) == 0 and L.ta_spk_affinity_ws_floats(6, 257) == 0
    assert L.ta_spk_lapmul_ws_floats(2048, 16) == L.ta_spk_lapmul_ws_floats(2048, 1) > 0 and L.ta_spk_lapmul_ws_floats(2048, 33) == 0
    assert L.ta_spk_lapmul_ws_floats(2048, 16) >= 8 * 2048 * 16                 # the columns are split: p = 16 fills the GPU
    assert L.ta_spk_gram_ws_floats(700, 48, 16) >= 48 * 16 and L.ta_spk_gram_ws_floats(700, 1025, 16) == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.ta_spk_affinity_f32(p, 5, 4, 5, p, 5, p, None, p, 7, None) == 1    # N < 6
    assert L.ta_spk_affinity_f32(p, 6, 4, 7, p, 6, p, None, p, 7, None) == 1    # keep > N
    assert L.ta_spk_affinity_f32(p, 6, 4, 6, p, 5, p, None, p, 7, None) == 1    # ldw < N
    assert L.ta_spk_affinity_f32(p, 6, 4, 6, p, 6, p, None, p, 8, None) == 1    # no such phase
    assert L.ta_spk_laplacian_matmul_f32(p, 6, p, p, 4, p, 4, 6, 33, p, None) == 1
    assert L.ta_spk_laplacian_matmul_f32(p, 6, p, p, 4, p, 4, 6, 4, None, None) == 1
    assert L.ta_spk_panel_update_f32(p, 33, 33, p, 4, 4, p, 33, 6, None) == 1   # b > 32
    assert L.ta_spk_panel_combine_f32(p, 4, 4, p, 4, 4, p, 4, 6, None) == 1     # Y == V


def test_operators_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    names = ("spk_affinity", "spk_laplacian_matmul", "spk_panel_gram", "spk_panel_update", "spk_panel_combine")
    assert set(names) <= set(torch_ops.OPERATORS)
    assert str(torch.ops.ta355.spk_affinity.default._schema).startswith("ta355::spk_affinity(Tensor embeddings, SymInt keep) -> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        W, deg, kept = torch.ops.ta355.spk_affinity(torch.empty(300, 192), 18)
        assert W.shape == (300, 300) and deg.shape == (300,) and kept.dtype == torch.int32
        X = torch.empty(300, 16)
        assert torch.ops.ta355.spk_laplacian_matmul(W, deg, X).shape == (300, 16)
        Cm = torch.ops.ta355.spk_panel_gram(torch.empty(300, 48), X)
        assert Cm.shape == (48, 16)
        assert torch.ops.ta355.spk_panel_update(X, torch.empty(300, 48), Cm).shape == (300, 16)
        assert torch.ops.ta355.spk_panel_combine(torch.empty(300, 48), Cm).shape == (300, 16)


def test_package_exports_the_device_clusterer():
    import tiny_audio_amd
    assert tiny_audio_amd.DeviceSpectralCluster is spectral.DeviceSpectralCluster


def test_dry_run_marshals_through_the_real_prototypes(dry):
    dry.calls.clear()
    E = torch.zeros(300, 192)
    W, deg, kept = ops.spk_affinity(E, ops.spk_keep(300, 0.06), want_kept=True)
    assert W.shape == (300, 300) and W.stride(0) == 300 and deg.shape == (300,) and kept.dtype == torch.int32
    W2, _, none = ops.spk_affinity(torch.zeros(257, 64), 15)
    assert W2.stride(0) == 260 and none is None                                 # rows padded to 4 floats
    wide = torch.zeros(300, 64)
    X = wide[:, 16:32]
    Y = ops.spk_laplacian_matmul(W, deg, X)
    Cm = ops.spk_panel_gram(wide[:, :48], X)
    assert Y.shape == (300, 16) and Cm.shape == (48, 16)
    assert ops.spk_panel_update(Y, wide[:, :48], Cm) is Y
    assert ops.spk_panel_combine(wide[:, :48], Cm, out=wide[:, 48:]).shape == (300, 16)
    assert dry.calls == ["ta_spk_affinity_f32", "ta_spk_affinity_f32", "ta_spk_laplacian_matmul_f32", "ta_spk_panel_gram_f32",
                         "ta_spk_panel_update_f32", "ta_spk_panel_combine_f32"]
    with pytest.raises(ValueError, match="32768"):
        ops.spk_affinity(torch.zeros(32769, 4), 6)
    with pytest.raises(AssertionError):
        ops.spk_laplacian_matmul(W, deg, wide.t()[:16].t().double())
    # the whole driver through the stubs: nothing is computed, so the start block cannot be orthonormalised and the host finishes
    dry.calls.clear()
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu", min_rows=64)
    Es, _ = R.embeddings(257, seed=257)
    np.random.seed(0)
    labels = d(Es.astype(np.float64))
    assert dry.calls[:2] == ["ta_spk_affinity_f32", "ta_spk_panel_gram_f32"] and d.last_info["path"] == "host" and len(labels) == 257


# ----------------------------------------------------------------------------- which path runs
def test_choose_k_and_trust():
    lam = np.array([0.0, 0.01, 0.02, 4.0, 5.0, 5.5, 6.0])
    assert spectral.choose_k(lam, np.full(7, 1e-4), 2, 5) == (3, True, pytest.approx(3.98), pytest.approx(1.0))
    assert spectral.choose_k(lam, np.full(7, 1e-4), 1, 5)[0] == R.eigengap_k(lam, 1, 5) == 3
    k, trusted, first, second = spectral.choose_k(np.array([0.0, 1.0, 2.001, 3.0]), np.full(4, 1e-3), 1, 3)
    assert k == 2 and not trusted and first - second == pytest.approx(0.001, abs=1e-9)     # 0.001 <= 4 * 1e-3
    assert spectral.choose_k(np.array([0.0, 1.0, 2.001, 3.0]), np.full(4, 1e-4), 1, 3)[1]  # 0.001 > 4 * 1e-4
    assert spectral.choose_k(np.array([0.0, 1.0, 2.0]), np.full(3, 0.5), 2, 2) == (2, True, 1.0, -np.inf)   # an oracle count: one gap


def test_small_inputs_take_the_host_path(cpu_ops):
    E, _ = R.embeddings(257, seed=257)
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu")
    np.random.seed(0)
    got = d(E.astype(np.float64))
    np.random.seed(0)
    want = SpectralCluster(2, 10)(E.astype(np.float64))
    assert np.array_equal(got, want) and d.last_info["path"] == "host" and "min_rows = 2048" in d.last_info["reason"]
    assert spectral.DeviceSpectralCluster().min_rows == spectral.MIN_ROWS == 2048 and spectral.DeviceSpectralCluster().seed == 0


def test_device_path_converges_on_the_emulated_operations(cpu_ops, monkeypatch):
    c = R.eig_case("5spk")
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu", min_rows=1024)
    W, deg = d.laplacian(c.E)
    a, b = d.smallest_eigenpairs(W, deg, 11), d.smallest_eigenpairs(W, deg, 11)
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1])              # the same seed gives the same basis
    assert a[3]["converged"] and (np.abs(a[0] - c.lam[:11]) <= a[2] + 1e-4).all()
    monkeypatch.setattr(d, "smallest_eigenpairs", lambda W, deg, m: a)         # the calls below decide on these pairs
    got = d(c.E.astype(np.float64))
    info = d.last_info
    assert info["path"] == "device" and info["converged"] and info["k"] == R.eigengap_k(c.lam, 2, 10) and info["max_residual"] <= info["tol"]
    assert R.same_partition(got, SpectralCluster(2, 10)(c.E.astype(np.float64)))
    assert len(set(d(c.E.astype(np.float64), oracle_num=3))) == 3 and d.last_info["k"] == 3       # an oracle count is used as given


def test_forced_non_convergence_hands_over_to_the_host(cpu_ops):
    c = R.eig_case("5spk")
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu", min_rows=1024, max_blocks=1)
    got = d(c.E.astype(np.float64))
    assert d.last_info["path"] == "host" and "not converged in 1 blocks" in d.last_info["reason"] and d.last_info["blocks"] == 1
    assert R.same_partition(got, SpectralCluster(2, 10)(c.E.astype(np.float64)))


def test_ambiguous_eigengap_hands_over_to_the_host(cpu_ops, monkeypatch):
    c = R.eig_case("5spk")
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu", min_rows=1024)
    real = d.smallest_eigenpairs

    def two_equal_gaps(W, deg, m):
        lam, vecs, res, info = real(W, deg, m)
        lam = lam.copy()
        lam[5] = lam[4] + (lam[4] - lam[3]) - 2 * res.max()                    # the second gap within 4 residuals of the widest
        return lam, vecs, res, info
    monkeypatch.setattr(d, "smallest_eigenpairs", two_equal_gaps)
    got = d(c.E.astype(np.float64))
    assert d.last_info["path"] == "host" and d.last_info["reason"].startswith("ambiguous eigengap")
    assert R.same_partition(got, SpectralCluster(2, 10)(c.E.astype(np.float64)))


def test_rank_deficient_block_ends_the_iteration(cpu_ops):
    """A graph of 80 disconnected pairs: L has two eigenvalues, so the Krylov space of any block is spent after two blocks."""
    N = 160
    W = torch.zeros(N, N)
    for i in range(0, N, 2):
        W[i, i + 1] = W[i + 1, i] = 1.0
    d = spectral.DeviceSpectralCluster(2, 10, device="cpu", min_rows=6)
    lam, vecs, res, info = d.smallest_eigenpairs(W, W.sum(1), 11)
    assert info["exhausted"] and info["blocks"] <= 3 and np.allclose(lam, 0.0, atol=1e-5) and res.max() < 1e-4


def test_clusterer_and_diarizer_arguments(cpu_ops, monkeypatch):
    """n == 0, n < 6 and ``device=None`` behave as before; ``cluster_device`` reaches the clusterer."""
    for dev in (None, "cpu"):
        sc = SpeakerClusterer(device=dev)
        assert sc(np.zeros((0, 4))).shape == (0,) and sc(np.ones((1, 4))).tolist() == [0] and sc(np.ones((5, 4))).tolist() == [0] * 5
        with pytest.raises(ValueError):
            sc(np.zeros(4))
    assert type(SpeakerClusterer()._get_spectral_cluster()) is SpectralCluster
    dsc = SpeakerClusterer(min_num_spks=3, max_num_spks=7, device="cpu")._get_spectral_cluster()
    assert isinstance(dsc, spectral.DeviceSpectralCluster) and (dsc.min_num_spks, dsc.max_num_spks, dsc.device) == (3, 7, "cpu")
    seen = []

    class Spy(SpeakerClusterer):
        def __init__(self, *a, **k):
            seen.append(k.get("device"))
            super().__init__(*a, **k)
    from tiny_audio_amd import diarization
    monkeypatch.setattr(diarization, "SpeakerClusterer", Spy)
    E, _ = R.embeddings(64, seed=64)

    class Stub:
        def embed_windows(self, buf, starts, lengths, window):
            return torch.from_numpy(E[:len(starts)])
    audio = np.zeros(16000 * 8, np.float32)
    frames = [True] * (len(audio) // 256 - 1)
    np.random.seed(0)
    a = LocalSpeakerDiarizer.diarize(audio, speaker_model=Stub(), speech_frames=frames)
    np.random.seed(0)
    b = SpeakerDiarizer.diarize(audio, speaker_model=Stub(), speech_frames=frames, cluster_device="cpu")
    assert seen == [None, "cpu"] and a == b and a                              # 50 windows: below min_rows, the host path either way
