"""LoRA dropout (peft ``lora_dropout`` p > 0) without a GPU: the mask definition's numpy twin, the model and checkpoint plumbing,
the call sequence under DRY_RUN (tests/test_dryrun_plumbing.py's stubs) and the ISA of the new kernels."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib
from tiny_audio_amd import lora_dropout as LD

ENC = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
LM = OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5])
def test_keep_rate_within_binomial_bounds(p):
    M, n = 512, 1024
    k = LD.keep_mask(p, 42, 7, 3, 1, M, n)
    q = 1.0 - LD.threshold(p) / 65536.0
    assert abs(LD.threshold(p) / 65536.0 - p) <= 2 ** -17          # the drop probability is p to 16 bits
    sd = np.sqrt(q * (1 - q) / k.size)
    assert abs(k.mean() - q) < 5 * sd, (k.mean(), q)
    rows = k.mean(1)                                                 # no row or column is special
    assert abs(rows - q).max() < 6 * np.sqrt(q * (1 - q) / n)
    assert LD.keep_mask(0.0, 42, 7, 3, 1, 4, 9).all()


def test_masks_of_members_layers_offsets_are_uncorrelated():
    p, M, n = 0.3, 256, 512
    base = LD.keep_mask(p, 9, 100, 2, 0, M, n).astype(np.float64)
    others = [LD.keep_mask(p, 9, 100, 2, 1, M, n), LD.keep_mask(p, 9, 100, 2, 2, M, n),        # q vs k, v: same input, own masks
              LD.keep_mask(p, 9, 100, 3, 0, M, n), LD.keep_mask(p, 9, 101, 2, 0, M, n),          # next layer, next offset
              LD.keep_mask(p, 9, 100 + (1 << 32), 2, 0, M, n), LD.keep_mask(p, 10, 100, 2, 0, M, n)]   # another rank, seed
    bound = 5.0 / np.sqrt(M * n)
    for o in others:
        c = np.corrcoef(base.ravel(), o.astype(np.float64).ravel())[0, 1]
        assert abs(c) < bound, c
    assert np.array_equal(LD.keep_mask(p, 9, 100, 2, 0, M, n), base.astype(bool))              # a pure function
    # rows of one column block and neighbouring column blocks are not copies of each other
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[:, :8], base[:, 8:16])


def test_numpy_twin_philox_known_answers():
    """Random123's philox4x32_10 known-answer vectors (the generator of ta_sample_f32 and the masks)."""
    assert [int(v) for v in LD.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(v) for v in LD.philox4x32_10(f, f, f, f, f, f)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_asr_model_with_lora_dropout_constructs_and_round_trips(tmp_path):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    m = ASRModel(ASRConfig(audio_config=ENC, text_config=LM, projector_hidden_dim=128, audio_token_id=999, use_lora=True,
                           lora_dropout=0.1), device="cpu", init="random")
    assert m.language_model.lora_dropout == 0.1
    out = tmp_path / "ck"
    m.save_pretrained(out)
    assert json.load(open(out / "adapter_config.json"))["lora_dropout"] == pytest.approx(0.1)
    b = ASRModel.from_pretrained(out, device="cpu", init="random", seed=9)
    assert b.config.lora_dropout == pytest.approx(0.1) and b.language_model.lora_dropout == pytest.approx(0.1)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            ASRModel(ASRConfig(audio_config=ENC, text_config=LM, use_lora=True, lora_dropout=bad), device="cpu", init="none")


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


class _Recorder:
    """Wraps the dry-run library: records the ta_lora_dropout descriptor each _ex call carries (p, seed, offset)."""

    def __init__(self, dry, monkeypatch):
        self.calls, self.drops = dry.calls, []
        for name, pos in (("ta_lm_forward_loss_ex", 18), ("ta_lm_backward_ex", 17)):
            stub = getattr(dry, name)

            def rec(*args, stub=stub, name=name, pos=pos):
                d = args[pos]._obj
                self.drops.append((name, round(d.p, 6), d.seed, d.offset))
                return stub(*args)
            monkeypatch.setattr(dry, name, rec, raising=False)


def _model_and_batch(p):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    cfg = ASRConfig(audio_config=ENC, text_config=LM, projector_hidden_dim=128, audio_token_id=999, use_lora=True,
                    freeze_projector=True, lora_dropout=p)
    m = ASRModel(cfg, device="cpu", init="random")
    ids, att, lab, counts = OW.synthetic_tokens(2, [12, 12], 1000, 999, 990, 991, n_text=10, n_suffix=4)
    meta = (torch.zeros(40, dtype=torch.int32), torch.zeros(40, dtype=torch.int64), 22)
    batch = dict(input_ids=torch.from_numpy(ids), input_features=torch.zeros(2, 128, 100), attention_mask=torch.from_numpy(att),
                 labels=torch.from_numpy(lab), audio_token_counts=torch.from_numpy(counts), label_meta=meta)
    return m, batch


def test_dropout_call_sequence(dry, monkeypatch):
    """Train mode: the _ex entry points carry p and a fresh offset per forward; F1, F2, B1, B2 hands each backward ITS forward's
    descriptor (kept by the autograd node, not by the module); eval() and generate() issue no dropout."""
    rec = _Recorder(dry, monkeypatch)
    m, batch = _model_and_batch(0.1)
    lm = m.language_model
    # ASRModel.train() keeps the frozen LM -- and with it peft's dropout modules -- in eval mode, as the reference's train() does
    # (tiny_audio/asr_modeling.py:344-357): no dropout until the LM itself is put in training mode
    m.train()
    with torch.no_grad():
        m(**batch)
    assert rec.drops == [] and lm.lora_drop_offset == 0
    lm.train(True)
    rec.calls.clear()
    o1 = m(**batch)
    o2 = m(**batch)
    o2.loss.backward()
    o1.loss.backward()
    seed = lm.lora_drop_seed
    assert rec.drops == [("ta_lm_forward_loss_ex", 0.1, seed, 0), ("ta_lm_forward_loss_ex", 0.1, seed, 1),
                         ("ta_lm_backward_ex", 0.1, seed, 1), ("ta_lm_backward_ex", 0.1, seed, 0)]
    assert "ta_lm_forward_loss" not in rec.calls and "ta_lm_backward" not in rec.calls
    m.eval()
    rec.calls.clear(); rec.drops.clear()
    with torch.no_grad():
        m(**batch)
    ids = torch.tensor([[5, 6] + [999] * 12 + [7, 8]] * 2)
    m.generate(input_ids=ids, input_features=torch.zeros(2, 128, 100), audio_attention_mask=torch.ones(2, 100, dtype=torch.int64),
               attention_mask=torch.ones_like(ids), max_new_tokens=3, eos_token_id=[])
    assert rec.drops == [] and "ta_lm_forward_loss" in rec.calls and "ta_lm_prefill" in rec.calls
    assert not any(c.endswith("_ex") for c in rec.calls)
    assert lm.lora_drop_offset == 2                                  # only training forwards draw


def test_backward_keeps_its_forward_stream_modes_behind_66_forwards(dry, monkeypatch):
    """The stream modes a tape was recorded in travel with its autograd node: 66 outstanding forwards, the modes flipped, and the
    backward of the FIRST forward still hands ta_lm_backward a handle in that forward's modes (a table of 64 tapes kept beside the
    module had forgotten it by then and read the tape in the new modes).  The next forward and its backward carry the new ones."""
    m, batch = _model_and_batch(0.0)
    lm = m.language_model
    seen = []
    stub = dry.ta_lm_backward

    def rec(*args):
        w = args[0]._obj                                             # the ta_lm_weights this backward was handed
        seen.append((w.res_f32, w.dx_f32))
        return stub(*args)
    monkeypatch.setattr(dry, "ta_lm_backward", rec, raising=False)
    m.train()
    outs = [m(**batch) for _ in range(66)]
    m.config.model_dtype = "float32"                                 # the owner's switch: the next forward runs in fp32 streams ...
    lm.res_f32 = lm.dx_f32 = True                                    # ... and this is what it sets on the LM
    outs[0].loss.backward()
    assert seen == [(0, 0)]
    assert lm.res_f32 and lm._w.res_f32 == 1 and lm._w.dx_f32 == 1  # the module is left as found
    m(**batch).loss.backward()
    assert seen[1:] == [(1, 1)]


def test_zero_dropout_issues_todays_calls(dry, monkeypatch):
    rec = _Recorder(dry, monkeypatch)
    seqs = []
    for p in (0.0, None):
        m, batch = _model_and_batch(0.0)
        if p is None:                                                # the behaviour before lora_dropout existed: the knob untouched
            m.language_model.lora_dropout = 0.0
        m.train()
        m.language_model.train(True)
        rec.calls.clear()
        m(**batch).loss.backward()
        seqs.append(list(rec.calls))
    assert seqs[0] == seqs[1] and "ta_lm_forward_loss" in seqs[0] and "ta_lm_backward" in seqs[0]
    assert rec.drops == [] and not any(c.endswith("_ex") for c in seqs[0])


def test_trainer_offsets_lora_dropout_per_rank(monkeypatch):
    from tiny_audio_amd import trainer as T
    m, _ = _model_and_batch(0.1)
    monkeypatch.setattr(T, "_distributed", lambda g: True)
    monkeypatch.setattr(T.dist, "get_rank", lambda g=None: 3)
    monkeypatch.setattr(T.dist, "get_world_size", lambda g=None: 4, raising=False)
    try:
        T.ASRTrainer(m, T.TrainingArguments())
    except Exception:                                                # the single-process box has no process group past this point
        pass
    assert m.language_model.lora_drop_offset == 3 << 32


def test_new_lora_kernels_use_no_scratch():
    """The masked kernels (csrc/lora.hip) keep everything in registers / LDS: ScratchSize 0 (test_isa_invariants.py's style)."""
    src = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "lora.hip")
    out = os.path.join(os.path.dirname(src), "build", "lora_isa.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [_lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only",
           "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    seen = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n.*?; ScratchSize: (\d+)", isa, re.S | re.M):
        seen[m.group(1)] = int(m.group(2))
    new = [k for k in seen if any(s in k for s in ("lora_skinny_nt_drop_kernel", "lora_tn_dual_drop_kernel", "lora_dx_drop_kernel",
                                                       "lora_keep_kernel"))]
    assert len(new) == 7, sorted(seen)
    assert all(seen[k] == 0 for k in new), {k: seen[k] for k in new}
