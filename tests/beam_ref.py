"""Reference for beam search (``ta_beam_topk_f32``, ``ta_beam_advance``, ``Qwen3MI355X.beam_decode``).  TEST CODE, numpy only.

HF ``GenerationMixin._beam_search`` (transformers 5.x, do_sample False) restated float32 operation by operation: the running beams of
``_get_running_beams_for_next_iteration``, the finished pool of ``_update_finished_beams`` with its three -1e9 maskings in HF's order,
``_check_early_stop_heuristic`` and the per-clip form of ``_beam_search_has_unfinished_sequences``.  tests/test_beam_ref.py pins it to
HF's own outputs (tests/golden/beam_search.npz); the GPU tests compare the kernels with it bit for bit.

Selections are stable (lowest index first on ties), as the device's are.  torch.topk promises no order among ties; the only ties that
occur in practice are between -1e9 sentinels, and those are never observable (a clip is done only when every pool slot is finished,
or at the maximum length, where the first K candidates all finish), so comparisons look at pool slots whose ``finished`` flag is set.

A done clip keeps stepping when the caller goes on (static shapes, as HF's batch does for its other clips): its pool cannot change any
more, because the maskings see to it.
"""
import numpy as np

F = np.float32
NEG = F(-1.0e9)


def n_candidates(num_beams, n_eos):
    return max(2, 1 + n_eos) * num_beams


def length_divisors(length_penalty, max_new):
    """d[n - 1] = float32(float(n) ** length_penalty), Python's pow as in HF."""
    return np.array([float(n) ** float(length_penalty) for n in range(1, max_new + 1)], np.float64).astype(F)


def topk_stable(acc, M):
    """acc f32 [B, N] -> (values [B, M], indices [B, M]): descending, lowest index first on ties (-inf included)."""
    idx = np.argsort(-acc.astype(F), axis=-1, kind="stable")[:, :M]
    return np.take_along_axis(acc, idx, -1), idx.astype(np.int64)


def candidates(rows, scores, M):
    """rows f32 [B * K, V] (processed log-probabilities), scores f32 [B, K] -> (cand_score f32 [B, M], cand_flat i64 [B, M])."""
    B, K = scores.shape
    V = rows.shape[1]
    acc = (rows.astype(F).reshape(B, K, V) + scores.astype(F)[:, :, None]).astype(F).reshape(B, K * V)
    return topk_stable(acc, M)


class BeamState:
    """The state of HF's loop for B clips, K beams, ``max_new`` new tokens (sequences hold the generated tokens only)."""

    def __init__(self, B, K, max_new, eos_ids=(), pad_id=0, length_penalty=1.0, early_stopping=False):
        assert early_stopping in (False, True, "never")
        self.B, self.K, self.max_new, self.eos, self.pad = B, K, max_new, [int(e) for e in eos_ids], int(pad_id)
        self.M = n_candidates(K, len(self.eos))
        self.lp, self.es = float(length_penalty), early_stopping
        self.div = length_divisors(length_penalty, max_new)
        self.t = 0
        self.run_seq = np.full((B, K, max_new), self.pad, np.int64)
        self.run_score = np.tile(np.array([0.0] + [-1.0e9] * (K - 1), F), (B, 1))
        self.parent = np.zeros((B, K), np.int64)
        self.next_ids = np.zeros((B, K), np.int64)
        self.pool_seq = np.full((B, K, max_new), self.pad, np.int64)
        self.pool_score = np.full((B, K), NEG, F)
        self.pool_len = np.zeros((B, K), np.int64)
        self.pool_fin = np.zeros((B, K), bool)
        self.heur = np.ones(B, bool)                  # is_early_stop_heuristic_unsatisfied
        self.done = np.zeros(B, bool)

    def step(self, cand_score, cand_flat, V):
        """One iteration from the M candidates of every clip (descending).  Returns the number of clips not done."""
        B, K, M, t = self.B, self.K, self.M, self.t
        assert t < self.max_new and cand_score.shape == (B, M)
        cs = np.asarray(cand_score, F)
        flat = np.asarray(cand_flat, np.int64)
        par, tok = flat // V, flat % V
        hit = np.isin(tok, self.eos) | (t + 1 == self.max_new)
        cand_seq = self.run_seq[np.arange(B)[:, None], par]                 # [B, M, max_new]: gathered BEFORE anything is written
        cand_seq[:, :, t] = tok
        # _get_running_beams_for_next_iteration
        rv = (cs + (hit.astype(F) * NEG).astype(F)).astype(F)
        _, ri = topk_stable(rv, K)
        take = lambda a, i: np.take_along_axis(a, i, 1)  # noqa: E731
        self.run_seq = cand_seq[np.arange(B)[:, None], ri]
        self.run_score = take(rv, ri)
        self.parent, self.next_ids = take(par, ri), take(tok, ri)
        # _update_finished_beams
        did = hit & (np.arange(M) < K)[None, :]
        fs = (cs / self.div[t]).astype(F)
        full = self.pool_fin.all(-1, keepdims=True) & (self.es is True)
        fs = (fs + (full.astype(F) * NEG).astype(F)).astype(F)
        fs = (fs + ((~self.heur)[:, None].astype(F) * NEG).astype(F)).astype(F)
        fs = (fs + ((~did).astype(F) * NEG).astype(F)).astype(F)
        m_score = np.concatenate([self.pool_score, fs], 1)
        fin_seq = cand_seq.copy()
        fin_seq[:, :, t + 1:] = self.pad
        m_seq = np.concatenate([self.pool_seq, fin_seq], 1)
        m_len = np.concatenate([self.pool_len, np.full((B, M), t + 1, np.int64)], 1)
        m_fin = np.concatenate([self.pool_fin, did], 1)
        _, pi = topk_stable(m_score, K)
        self.pool_seq = m_seq[np.arange(B)[:, None], pi]
        self.pool_score, self.pool_len, self.pool_fin = take(m_score, pi), take(m_len, pi), take(m_fin, pi)
        # _check_early_stop_heuristic (cur_len has advanced) and _beam_search_has_unfinished_sequences, per clip
        hd = self.div[self.max_new - 1] if (self.es == "never" and self.lp > 0.0) else self.div[t]
        best = (self.run_score[:, :1] / hd).astype(F)
        worst = np.where(self.pool_fin, self.pool_score.min(-1, keepdims=True), NEG)
        self.heur = self.heur & (best > worst).any(-1)
        cont = self.heur & ~(self.pool_fin.all(-1) & (self.es is True)) & ~hit.all(-1)
        self.done = self.done | ~cont
        self.t = t + 1
        return int((~self.done).sum())

    def step_rows(self, rows, V=None):
        """One iteration from the processed log-probability rows f32 [B * K, V] of the running beams."""
        V = rows.shape[1] if V is None else V
        cs, cf = candidates(np.asarray(rows, F)[:, :V], self.run_score, self.M)
        return self.step(cs, cf, V)

    def result(self, num_return_sequences=1):
        """-> (sequences i64 [B * n, n_new], scores f32 [B * n]) as HF crops them (generated tokens only)."""
        n = num_return_sequences
        n_new = int(self.pool_len[:, :n].max()) if self.B else 0
        return self.pool_seq[:, :n, :n_new].reshape(self.B * n, n_new), self.pool_score[:, :n].reshape(-1)


def run_rows(step_rows, B, K, max_new, V, **kw):
    """Drive a BeamState with per-step rows ``step_rows[t]`` [B * K, V] until every clip is done, as HF's loop does when its batch-wide
    condition and the per-clip one coincide (B == 1, or the caller keeps stepping)."""
    st = BeamState(B, K, max_new, **kw)
    for rows in step_rows:
        if st.step_rows(rows, V) == 0:
            break
    return st
