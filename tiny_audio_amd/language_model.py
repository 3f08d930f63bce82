"""Frozen causal LM on MI355X (drop-in for ``ASRModel.language_model`` on the training path): Qwen3, or a SmolLM3 / Llama-style
decoder -- no q_norm / k_norm, per-layer NoPE (``LMConfig.qk_norm`` / ``no_rope_layers``; TF:models/smollm3/modeling_smollm3.py:174-250).

Reference: ``Qwen3ForCausalLM.forward`` TF:models/qwen3/modeling_qwen3.py:448-508 + ``ForCausalLMLoss``
TF:loss/loss_utils.py:33-71, called at tiny_audio/asr_modeling.py:517-526 with frozen weights
(``requires_grad_(False)``, :251-253), so backward is activation-gradient only.

Every frozen matrix is kept twice in bf16 -- [out,in] for the forward GEMM and [in,out] for dX = dY W --
so both directions run the same NT MFMA kernel (288 GB of HBM: the second copy costs 1.2 GB).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib, decoding
from .asr_config import LMConfig
from .ops import BF16, F32, ptr, stream


def _pad128(n):
    return (n + 127) // 128 * 128


# LoRA adapters of linears that share an input are stacked into one GROUP (csrc/lora.hip): group -> peft target names
LORA_GROUPS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("o", ("self_attn.o_proj",)),
               ("gu", ("mlp.gate_proj", "mlp.up_proj")), ("d", ("mlp.down_proj",)))


NO_NORM_FULL_FT = ("full decoder fine-tuning (freeze_language_model=False) of a text tower without q/k-norm (smollm3, llama) is not "
                   "built: the trainable-LM masters and gradient slots include q_norm / k_norm; train it with LoRA (use_lora=True)")


class Qwen3MI355X(torch.nn.Module):
    def __init__(self, config: LMConfig, device="cuda"):
        super().__init__()
        self.config = config
        self.device_ = torch.device(device)
        self.vocab_pad = _pad128(config.vocab_size)
        self._bufs = {}
        self._w = None
        self._layers_arr = None
        self.lora_rank = 0
        self.lora_groups = 0
        self.lora_targets = set()
        self.lora_dropout = 0.0
        self.lora_drop_seed = 0
        self.lora_drop_offset = 0        # Philox offset of the next training forward (ASRTrainer adds rank << 32 on DDP ranks)
        self._lora_bound = None
        self.train_base = False          # full decoder fine-tuning (freeze_language_model=False)
        self.want_train_base = False     # ... requested before the weights exist: enabled by _finalize
        self._ft_bound = None
        self._ft_versions = None
        self.accumulate_into_grad = False   # trainer opt-in: weight gradients are added straight into Parameter.grad
        self._res_f32 = self._dx_f32 = False   # storage of the residual / d(x) streams (ta_lm_weights.res_f32 / dx_f32): bf16

    # ------------------------------------------------------------------ LoRA (stage 2; asr_modeling.py:289-301)
    # storage of the forward residual stream (+ its tape rows) and of the backward d(x) stream: fields of THIS model's weights handle
    # (include/ta355.h, ABI 4) -- rounds 1-5 kept them in process-wide library state
    @property
    def res_f32(self) -> bool:
        return self._res_f32

    @res_f32.setter
    def res_f32(self, v):
        self._res_f32 = bool(v)
        if self._w is not None:
            self._w.res_f32 = int(self._res_f32)

    @property
    def dx_f32(self) -> bool:
        return self._dx_f32

    @dx_f32.setter
    def dx_f32(self, v):
        self._dx_f32 = bool(v)
        if self._w is not None:
            self._w.dx_f32 = int(self._dx_f32)

    def _lora_dims(self):
        """group -> [(peft target, out_features)], in_features"""
        c = self.config
        D, F, nq, nkv, hd = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim
        outs = {"self_attn.q_proj": nq * hd, "self_attn.k_proj": nkv * hd, "self_attn.v_proj": nkv * hd,
                "self_attn.o_proj": D, "mlp.gate_proj": F, "mlp.up_proj": F, "mlp.down_proj": D}
        ins = {"qkv": D, "o": nq * hd, "gu": D, "d": F}
        return {g: ([(t, outs[t]) for t in ts], ins[g]) for g, ts in LORA_GROUPS}

    def lora_parameters(self):
        return [getattr(self, f"lora_{ab}_{g}") for g, _ in LORA_GROUPS for ab in ("la", "lb")] if self.lora_rank else []

    @torch.no_grad()
    def enable_lora(self, rank=8, alpha=32, dropout=0.0, target_modules=None, seed=0):
        """peft ``LoraConfig(r, lora_alpha, target_modules, bias='none')`` on every decoder layer (tiny_audio/asr_modeling.py:289-301,
        defaults tiny_audio/asr_config.py:72-75: r = 8, alpha = 32, all 7 linears): lora_A ~ kaiming_uniform(a=sqrt(5)) =
        U(+-1/sqrt(in)), lora_B = 0, y += (alpha/r) B A x.  The trainable fp32 masters are 8 Parameters [n_layers, ...] in the
        stacked group layout of include/ta355.h.

        ``rank``: any r with 3 r <= 64 (the q|k|v group's three adapters share one 64-wide K tile).
        ``dropout``: peft's ``lora_dropout`` p, 0 <= p < 1: in training mode each adapted linear drops its adapter input with its
        own mask (include/ta355.h ``ta_lora_dropout``; masks drawn per training forward from ``seed``); evaluation and decoding
        never apply it.
        ``target_modules``: any subset of the 7 linears (peft suffix names).  A group none of whose members is targeted is
        switched off in the C library (``ta_lm_weights.lora_groups``); inside a live group the members that are not targeted
        keep A = B = 0, which makes both of their gradients exactly zero (dA = s (dy B)^T x, dB = dy^T (x A^T)), so AdamW
        never moves them; ``export_lora_state_dict`` / ``lora_param_count`` only see the targeted ones."""
        if self.train_base or self.want_train_base:
            raise NotImplementedError("LoRA on top of a trainable base LM is not built")
        if not (1 <= int(rank) and 3 * int(rank) <= 64):
            raise NotImplementedError("lora_rank must satisfy 3 * rank <= 64 (one 64-wide K tile per adapter group)")
        dropout = float(dropout or 0.0)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"lora_dropout must satisfy 0 <= p < 1, got {dropout}")
        all_t = [t for _, ts in LORA_GROUPS for t in ts]
        if target_modules is None:
            targets = set(all_t)
        else:
            short = {t.split(".")[-1]: t for t in all_t}
            unknown = [t for t in target_modules if t.split(".")[-1] not in short]
            if unknown or not list(target_modules):
                raise ValueError(f"lora_target_modules {unknown or '[]'}: expected a non-empty subset of {sorted(short)}")
            targets = {short[t.split(".")[-1]] for t in target_modules}
        rank = int(rank)
        Lyr, dev = self.config.num_hidden_layers, self.device_
        gen = torch.Generator(device="cpu"); gen.manual_seed(seed)
        self.lora_groups = 0
        for gi, (g, (members, fin)) in enumerate(self._lora_dims().items()):
            bound = 1.0 / math.sqrt(fin)
            a = (torch.rand((Lyr, len(members) * rank, fin), generator=gen, dtype=F32) * 2 - 1) * bound
            for j, (t, _) in enumerate(members):
                if t not in targets:
                    a[:, j * rank:(j + 1) * rank] = 0
                else:
                    self.lora_groups |= 1 << gi
            b = torch.zeros((Lyr, sum(o for _, o in members), rank), dtype=F32)
            setattr(self, f"lora_la_{g}", torch.nn.Parameter(a.to(dev)))
            setattr(self, f"lora_lb_{g}", torch.nn.Parameter(b.to(dev)))
        self.lora_rank, self.lora_alpha, self.lora_targets = rank, alpha, targets
        self.lora_dropout = dropout
        self.lora_drop_seed = (0x10DA_D809 * (int(seed) + 1)) & 0x7FFFFFFFFFFFFFFF
        self.lora_drop_offset = 0
        self._lora_bound = None
        self._finalize_lora_scale()
        return self

    def next_lora_dropout(self):
        """(p, seed, offset) for the next forward: a fresh offset per TRAINING forward with p > 0; None otherwise (evaluation,
        p == 0, no adapters).  The backward must be handed the same triple (the autograd node keeps it)."""
        if not (self.lora_rank and self.lora_dropout > 0.0 and self.training):
            return None
        off = self.lora_drop_offset
        self.lora_drop_offset += 1
        return (float(self.lora_dropout), int(self.lora_drop_seed), int(off))

    def lora_param_count(self):
        """peft's trainable-parameter count: r (in + out) per targeted linear and layer (the stacked masters also hold the
        zero blocks of members that are not targeted)."""
        if not self.lora_rank:
            return 0
        n = 0
        for g, (members, fin) in self._lora_dims().items():
            n += sum(self.lora_rank * (fin + o) for t, o in members if t in self.lora_targets)
        return n * self.config.num_hidden_layers

    def _finalize_lora_scale(self):
        if self._w is not None and self.lora_rank:
            self._w.lora_rank, self._w.lora_scale = self.lora_rank, float(self.lora_alpha) / self.lora_rank
            self._w.lora_groups = self.lora_groups

    @torch.no_grad()
    def load_lora_state_dict(self, sd):
        """Accepts peft adapter naming (``...model.layers.N.self_attn.q_proj.lora_A[.default].weight``) or the bare
        ``model.layers.N.<target>.lora_A`` keys of oracle/weights.py:init_lora."""
        r = self.lora_rank
        found = {}
        for k, v in sd.items():
            k2 = k.replace(".default", "")
            if k2.endswith(".weight"):
                k2 = k2[: -len(".weight")]
            i = k2.find("layers.")
            if i >= 0 and (k2.endswith(".lora_A") or k2.endswith(".lora_B")):
                found[k2[i:]] = torch.as_tensor(v).to(dtype=F32)
        for g, (members, fin) in self._lora_dims().items():
            la, lb = getattr(self, f"lora_la_{g}"), getattr(self, f"lora_lb_{g}")
            for i in range(self.config.num_hidden_layers):
                row = 0
                for j, (t, o) in enumerate(members):
                    if t in self.lora_targets:
                        la.data[i, j * r:(j + 1) * r].copy_(found[f"layers.{i}.{t}.lora_A"])
                        lb.data[i, row:row + o].copy_(found[f"layers.{i}.{t}.lora_B"])
                    row += o
        return self

    def export_lora_state_dict(self, prefix="base_model.model.model.", suffix=".weight"):
        """peft adapter_model naming by default; ``prefix='model.', suffix=''`` gives the oracle's keys."""
        r, sd = self.lora_rank, {}
        for g, (members, fin) in self._lora_dims().items():
            la, lb = getattr(self, f"lora_la_{g}").detach(), getattr(self, f"lora_lb_{g}").detach()
            for i in range(self.config.num_hidden_layers):
                row = 0
                for j, (t, o) in enumerate(members):
                    if t in self.lora_targets:
                        sd[f"{prefix}layers.{i}.{t}.lora_A{suffix}"] = la[i, j * r:(j + 1) * r].clone()
                        sd[f"{prefix}layers.{i}.{t}.lora_B{suffix}"] = lb[i, row:row + o].clone()
                    row += o
        return sd

    def _bind_lora(self):
        """Point the per-layer struct fields at the current storage of the 8 master Parameters (a flat-buffer
        optimizer may have re-homed ``.data`` since the last call)."""
        ps = self.lora_parameters()
        key = tuple(p.data_ptr() for p in ps)
        if key == self._lora_bound:
            return
        for p in ps:
            assert p.dtype == F32 and p.is_contiguous()
        for g, _ in LORA_GROUPS:
            for ab in ("la", "lb"):
                p = getattr(self, f"lora_{ab}_{g}")
                step = p[0].numel() * 4
                for i in range(self.config.num_hidden_layers):
                    setattr(self._layers_arr[i], f"{ab}_{g}", p.data_ptr() + i * step)
        self._lora_bound = key

    # ------------------------------------------------------------------ full decoder fine-tuning (8(f) rank 4)
    # (kind, per-layer struct field or None, needs bf16 images, decays)
    FT_KINDS = (("wqkv", True), ("wo", True), ("wgu", True), ("wd", True), ("ln_in_w", False), ("ln_post_w", False),
                ("qn_w", False), ("kn_w", False))

    def ft_parameters(self):
        """The fp32 masters of the trainable LM: 8 stacked per-layer Parameters [n_layers, ...] + final norm + embedding."""
        if not self.train_base:
            return []
        return [getattr(self, "ft_" + k) for k, _ in self.FT_KINDS] + [self.ft_norm_w, self.ft_embed]

    @torch.no_grad()
    def enable_full_finetune(self):
        """freeze_language_model=False (tiny_audio/asr_config.py:77; configs/experiments/embedded.yaml:23): every LM weight
        trains.  Masters are fp32 Parameters (stacked over the layers, q|k|v and gate|up fused like the kernels' images);
        the kernels keep reading bf16 images (W and W^T) that ``refresh_images`` rebuilds after an optimizer step, the
        norm scales and the embedding table are read from the masters directly."""
        if self.lora_rank:
            raise NotImplementedError("LoRA on top of a trainable base LM is not built")
        if not self.config.qk_norm:
            raise NotImplementedError(NO_NORM_FULL_FT)
        if self._w is None:
            raise _lib.Ta355Error("load or initialise the LM weights before enable_full_finetune()")
        c, b = self.config, self._bufs
        Lyr = c.num_hidden_layers
        src = getattr(self, "_fp32_src", None) or {}
        for kind, _img in self.FT_KINDS:
            rows = [src.get(f"layers.{i}.{kind}", b[f"layers.{i}.{kind}"]).to(F32) for i in range(Lyr)]
            p = torch.nn.Parameter(torch.stack(rows, 0).contiguous())
            p._no_decay = not _img                      # norm scales: the no-decay group (scripts/train.py:397-432)
            setattr(self, "ft_" + kind, p)
        self.ft_norm_w = torch.nn.Parameter(b["norm_w"].to(F32).clone()); self.ft_norm_w._no_decay = True
        self.ft_embed = torch.nn.Parameter(b["embed_f32"].clone())
        self._fp32_src = None
        self.train_base = True
        self._w.train_base = 1
        self._ft_bound = self._ft_versions = None
        self._bind_ft()
        return self

    def _bind_ft(self):
        """Point the kernels at the masters they read directly (norm scales, embedding) -- a flat-buffer optimizer may have
        re-homed ``.data`` -- and rebuild the bf16 images if any master changed since they were built."""
        ps = self.ft_parameters()
        key = tuple(p.data_ptr() for p in ps)
        if key != self._ft_bound:
            for p in ps:
                assert p.dtype == F32 and p.is_contiguous()
            for kind in ("ln_in_w", "ln_post_w", "qn_w", "kn_w"):
                p = getattr(self, "ft_" + kind)
                step = p[0].numel() * 4
                for i in range(self.config.num_hidden_layers):
                    setattr(self._layers_arr[i], kind, p.data_ptr() + i * step)
            self._w.norm_w = self.ft_norm_w.data_ptr()
            self._w.embed_f32 = self.ft_embed.data_ptr()
            # the buffer table follows the masters too (the initial copies are dropped: the embedding alone is 0.6 GB)
            b = self._bufs
            b["embed_f32"], b["norm_w"] = self.ft_embed.data, self.ft_norm_w.data
            for kind in ("ln_in_w", "ln_post_w", "qn_w", "kn_w"):
                m = getattr(self, "ft_" + kind).data
                for i in range(self.config.num_hidden_layers):
                    b[f"layers.{i}.{kind}"] = m[i]
            self._ft_bound = key
            self._ft_versions = None
        ver = tuple(p._version for p in ps)
        if ver != self._ft_versions:
            self.refresh_images()

    @torch.no_grad()
    def refresh_images(self):
        """bf16 W / W^T images of the four matrices of every layer and of the tied embedding, from the fp32 masters
        (in place: the kernels' pointers stay valid).  Call after every optimizer step that writes the masters through
        raw pointers; torch optimizers are detected through the Parameters' version counters."""
        b = self._bufs
        gpu = self.device_.type == "cuda" and not _lib.DRY_RUN
        L_ = _lib.lib() if gpu else None

        def images(master, wb, wt):                      # fp32 [N, K] -> bf16 [N, K] and bf16 [K, N]
            if not gpu:
                wb.copy_(master); wt[:, :master.shape[0]].copy_(wb.t()); return
            N, K = master.shape
            _lib.check(L_.ta_cast_f32_bf16(ptr(master), ptr(wb), master.numel(), stream()), "ta_cast_f32_bf16")
            _lib.check(L_.ta_transpose_to_bf16(ptr(master), 1, K, 0, 0, ptr(wt), wt.shape[1], N, K, stream()), "ta_transpose_to_bf16")
        for kind, img in self.FT_KINDS:
            if not img:
                continue
            m = getattr(self, "ft_" + kind)
            for i in range(self.config.num_hidden_layers):
                images(m[i], b[f"layers.{i}.{kind}"], b[f"layers.{i}.{kind}_t"])
        V = self.config.vocab_size
        images(self.ft_embed, b["embed_bf16"][:V], b["embed_t_bf16"])       # rows V..vocab_pad stay zero in both images
        self._ft_versions = tuple(p._version for p in self.ft_parameters())

    def ft_state_dict_hf(self):
        """The masters under the reference's parameter names (``model.layers.N.self_attn.q_proj.weight`` ...; tiny_audio/asr_modeling.py:409-421;
        the tied ``lm_head.weight`` alias of the embedding is not repeated: safetensors refuses shared storage)."""
        c = self.config
        nq, nkv, hd, F_ = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size
        sd = {"model.embed_tokens.weight": self.ft_embed.detach(), "model.norm.weight": self.ft_norm_w.detach()}
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}."
            a = p + "self_attn."
            w = self.ft_wqkv.detach()[i]
            sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"] = w[: nq * hd], w[nq * hd:(nq + nkv) * hd], w[(nq + nkv) * hd:]
            sd[a + "o_proj.weight"] = self.ft_wo.detach()[i]
            gu = self.ft_wgu.detach()[i]
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = gu[:F_], gu[F_:]
            sd[p + "mlp.down_proj.weight"] = self.ft_wd.detach()[i]
            sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = self.ft_ln_in_w.detach()[i], self.ft_ln_post_w.detach()[i]
            sd[a + "q_norm.weight"], sd[a + "k_norm.weight"] = self.ft_qn_w.detach()[i], self.ft_kn_w.detach()[i]
        return sd

    @torch.no_grad()
    def load_ft_state_dict_hf(self, sd):
        """Inverse of ``ft_state_dict_hf`` (keys may carry a ``language_model.`` prefix; ``lm_head.weight`` is ignored:
        it is the embedding)."""
        c = self.config
        g = lambda k: torch.as_tensor(sd[k] if k in sd else sd["language_model." + k]).to(device=self.device_, dtype=F32)
        self.ft_embed.copy_(g("model.embed_tokens.weight")); self.ft_norm_w.copy_(g("model.norm.weight"))
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}."
            a = p + "self_attn."
            self.ft_wqkv[i].copy_(torch.cat([g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight")], 0))
            self.ft_wo[i].copy_(g(a + "o_proj.weight"))
            self.ft_wgu[i].copy_(torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0))
            self.ft_wd[i].copy_(g(p + "mlp.down_proj.weight"))
            self.ft_ln_in_w[i].copy_(g(p + "input_layernorm.weight")); self.ft_ln_post_w[i].copy_(g(p + "post_attention_layernorm.weight"))
            self.ft_qn_w[i].copy_(g(a + "q_norm.weight")); self.ft_kn_w[i].copy_(g(a + "k_norm.weight"))
        self.refresh_images()
        return self

    # ------------------------------------------------------------------ weights
    def _rope_tables(self):
        c = self.config
        inv = 1.0 / (c.rope_theta ** (torch.arange(0, c.head_dim, 2, dtype=torch.float32) / c.head_dim))  # modeling_qwen3.py:117
        freqs = torch.arange(c.max_position_embeddings, dtype=torch.float32)[:, None] * inv[None, :]
        return freqs.cos().contiguous(), freqs.sin().contiguous()

    keep_fp32 = False     # set before loading weights that will be fine-tuned: the fp32 originals seed the masters

    def _pack_matrix(self, name, w):
        """w fp32 [out, in] on device -> bf16 copy + transposed bf16 copy."""
        if self.keep_fp32:
            if getattr(self, "_fp32_src", None) is None:
                self._fp32_src = {}
            self._fp32_src[name] = w
        wb = w.to(BF16).contiguous()
        self._bufs[name] = wb
        self._bufs[name + "_t"] = wb.t().contiguous()

    def _set_embedding(self, emb):
        c, dev = self.config, self.device_
        V, D = emb.shape
        # Hub checkpoints carry padded embedding matrices (Qwen3-0.6B / 1.7B: 151 936 rows); the reference calls
        # resize_token_embeddings(len(tokenizer)) after adding <audio> (tiny_audio/asr_modeling.py:160-171), which keeps
        # the FIRST vocab_size rows -- row vocab_size-1 becomes the <audio> token.  Do the same here.
        if D != c.hidden_size or V < c.vocab_size:
            raise ValueError(f"embed_tokens is [{V}, {D}]; the config needs at least [{c.vocab_size}, {c.hidden_size}]")
        if V > c.vocab_size:
            emb = emb[: c.vocab_size]
            V = c.vocab_size
        self._bufs["embed_f32"] = emb.to(device=dev, dtype=F32).contiguous()
        eb = torch.zeros((self.vocab_pad, D), device=dev, dtype=BF16)
        eb[:V] = self._bufs["embed_f32"].to(BF16)
        self._bufs["embed_bf16"] = eb
        self._bufs["embed_t_bf16"] = eb.t().contiguous()

    def _check_norm_keys(self, sd, prefix=""):
        """A q/k-norm tower (Qwen3) needs ``self_attn.q_norm.weight`` / ``k_norm.weight`` of every layer; a tower without (SmolLM3,
        Llama) must not be handed any: either mistake would otherwise run the wrong arithmetic silently."""
        for i in range(self.config.num_hidden_layers):
            for n in ("q_norm", "k_norm"):
                k = f"model.layers.{i}.self_attn.{n}.weight"
                has = (prefix + k) in sd or k in sd
                if self.config.qk_norm and not has:
                    raise KeyError(f"{k} is missing: a {self.config.model_type} text tower has q/k-norm")
                if has and not self.config.qk_norm:
                    raise KeyError(f"{k}: a {self.config.model_type} text tower has no q/k-norm (text_config.model_type is wrong for this checkpoint)")

    def load_state_dict_hf(self, sd):
        """sd: {``model.layers.N.self_attn.q_proj.weight`` ...: array-like fp32} in the reference's naming (SmolLM3 / Llama: the same
        names minus ``q_norm`` / ``k_norm``)."""
        c, dev = self.config, self.device_
        g = lambda k: torch.as_tensor(sd[k]).to(device=dev, dtype=F32)
        self._check_norm_keys(sd)
        self._bufs = {}
        self._set_embedding(g("model.embed_tokens.weight"))
        self._bufs["norm_w"] = g("model.norm.weight").contiguous()
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}."
            q = f"layers.{i}."
            a = p + "self_attn."
            self._pack_matrix(q + "wqkv", torch.cat([g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight")], 0))
            self._pack_matrix(q + "wo", g(a + "o_proj.weight"))
            self._pack_matrix(q + "wgu", torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0))
            self._pack_matrix(q + "wd", g(p + "mlp.down_proj.weight"))
            self._bufs[q + "ln_in_w"] = g(p + "input_layernorm.weight").contiguous()
            self._bufs[q + "ln_post_w"] = g(p + "post_attention_layernorm.weight").contiguous()
            if c.qk_norm:
                self._bufs[q + "qn_w"] = g(a + "q_norm.weight").contiguous()
                self._bufs[q + "kn_w"] = g(a + "k_norm.weight").contiguous()
        self._finalize()
        return self

    @torch.no_grad()
    def random_init(self, seed=1):
        c, dev = self.config, self.device_
        D, F, V = c.hidden_size, c.intermediate_size, c.vocab_size
        nq, nkv, hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        gen = torch.Generator(device=dev); gen.manual_seed(seed)
        rn = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=gen, dtype=F32) * std
        self._bufs = {}
        self._set_embedding(rn(V, D, std=1 / math.sqrt(D)))
        self._bufs["norm_w"] = 1 + rn(D, std=0.1)
        for i in range(c.num_hidden_layers):
            q = f"layers.{i}."
            self._pack_matrix(q + "wqkv", rn((nq + 2 * nkv) * hd, D, std=1 / math.sqrt(D)))
            self._pack_matrix(q + "wo", rn(D, nq * hd, std=0.5 / math.sqrt(nq * hd)))
            self._pack_matrix(q + "wgu", rn(2 * F, D, std=1 / math.sqrt(D)))
            self._pack_matrix(q + "wd", rn(D, F, std=0.5 / math.sqrt(F)))
            self._bufs[q + "ln_in_w"] = 1 + rn(D, std=0.1)
            self._bufs[q + "ln_post_w"] = 1 + rn(D, std=0.1)
            if c.qk_norm:
                self._bufs[q + "qn_w"] = 1 + rn(hd, std=0.1)
                self._bufs[q + "kn_w"] = 1 + rn(hd, std=0.1)
        self._finalize()
        return self

    def _finalize(self):
        c, b, dev = self.config, self._bufs, self.device_
        cos, sin = self._rope_tables()
        b["rope_cos"], b["rope_sin"] = cos.to(dev), sin.to(dev)
        L = c.num_hidden_layers
        arr = (_lib.LmLayer * L)()
        for i in range(L):
            for f, _ in _lib.LmLayer._fields_:
                if f in ("qn_w", "kn_w") and not c.qk_norm:
                    continue                                   # NULL = no q/k-norm (include/ta355.h ta_lm_layer)
                if not f.startswith(("la_", "lb_")):
                    setattr(arr[i], f, b[f"layers.{i}.{f}"].data_ptr())
        w = _lib.LmWeights(vocab=c.vocab_size, vocab_pad=self.vocab_pad, hidden=c.hidden_size, ffn=c.intermediate_size,
                           n_layers=L, heads=c.num_attention_heads, kv_heads=c.num_key_value_heads, head_dim=c.head_dim,
                           max_pos=c.max_position_embeddings, eps=c.rms_norm_eps, res_f32=int(self._res_f32),
                           dx_f32=int(self._dx_f32), nope_layers=c.nope_mask)
        for f in ("embed_f32", "embed_bf16", "embed_t_bf16", "norm_w", "rope_cos", "rope_sin"):
            setattr(w, f, b[f].data_ptr())
        w.layers = C.cast(arr, C.POINTER(_lib.LmLayer))
        self._layers_arr, self._w, self._lora_bound = arr, w, None
        self._finalize_lora_scale()
        if self.train_base or self.want_train_base:      # (re)seed the masters from the weights just loaded
            self.train_base = False
            self.enable_full_finetune()

    def export_state_dict_hf(self):
        """Back to the reference's parameter names as fp32 numpy (used by bench.py's CPU-baseline leg)."""
        c, b = self.config, self._bufs
        nq, nkv, hd, F = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size
        f = lambda t: t.detach().float().cpu().numpy()
        if self.train_base:                       # fine-tuned: the fp32 masters, not the bf16 images
            return {k: f(v) for k, v in self.ft_state_dict_hf().items()}
        sd = {"model.embed_tokens.weight": f(b["embed_f32"]), "model.norm.weight": f(b["norm_w"])}
        for i in range(c.num_hidden_layers):
            p, q = f"model.layers.{i}.", f"layers.{i}."
            a = p + "self_attn."
            w = f(b[q + "wqkv"])
            sd[a + "q_proj.weight"], sd[a + "k_proj.weight"] = w[: nq * hd], w[nq * hd:(nq + nkv) * hd]
            sd[a + "v_proj.weight"] = w[(nq + nkv) * hd:]
            sd[a + "o_proj.weight"] = f(b[q + "wo"])
            gu = f(b[q + "wgu"])
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = gu[:F], gu[F:]
            sd[p + "mlp.down_proj.weight"] = f(b[q + "wd"])
            sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = f(b[q + "ln_in_w"]), f(b[q + "ln_post_w"])
            if c.qk_norm:
                sd[a + "q_norm.weight"], sd[a + "k_norm.weight"] = f(b[q + "qn_w"]), f(b[q + "kn_w"])
        return sd

    def get_input_embeddings_weight(self):
        return self._bufs["embed_f32"]

    @torch.no_grad()
    def set_embedding_weight(self, weight):
        """Replace the tied token embedding (``set_input_embeddings`` / ``set_output_embeddings`` of the reference,
        tiny_audio/asr_modeling.py:372-382): the fp32 lookup table and both bf16 lm_head images are rebuilt and the weights
        handle re-pointed.  With a trainable base LM the fp32 master takes the values and the images follow at the next forward."""
        w = torch.as_tensor(weight).detach()
        if self.train_base:
            self.ft_embed.copy_(w[: self.config.vocab_size].to(self.ft_embed))
            self._ft_versions = None
            return
        self._set_embedding(w)
        if self._w is not None:
            for f in ("embed_f32", "embed_bf16", "embed_t_bf16"):
                setattr(self._w, f, self._bufs[f].data_ptr())

    # ------------------------------------------------------------------ raw forward / backward (no autograd)
    def forward_loss(self, input_ids, src_row, audio, kmask, label_rows, label_targets, n_label_rows, loss_scale,
                     want_logits=False, pos=None, lora_dropout=None, seg=None, label_smoothing=0.0, z_loss=0.0):
        """Returns (loss[1] f32, nll[n] f32, logits or None, ctx) -- ctx feeds ``backward_from_ctx``.
        ``label_smoothing`` (HF label_smoothing_factor, 0 <= eps < 1) and ``z_loss`` (coefficient of logsumexp^2 per target row,
        >= 0): the loss options of include/ta355.h ``ta_ce_options``, computed inside the cross-entropy launch.  With either set,
        ``loss`` is the objective and ctx["obj"] its per-row terms; ``nll`` stays the plain NLL, and the backward needs nothing new
        (the tape's dlogits are the objective's).  Both 0: the call without options.
        ``lora_dropout``: (p, seed, offset) of ``next_lora_dropout()`` or None; kept in ctx for the backward.
        ``seg``: int32 [2, B*L], the table of ``ops.segment_table`` for packed rows (several clips per row, block-diagonal
        attention), or None; kept in ctx for the backward too."""
        if self._w is None:
            raise _lib.Ta355Error("LM weights not loaded")
        eps, zc = check_loss_options(label_smoothing, z_loss)
        L_ = _lib.lib()
        B, L = input_ids.shape
        dev = self.device_
        if self.lora_rank:
            self._bind_lora()
        if self.train_base:
            self._bind_ft()
        tape = torch.empty(L_.ta_lm_tape_bytes(C.byref(self._w), B, L, n_label_rows), device=dev, dtype=torch.uint8)
        ws = torch.empty(L_.ta_lm_workspace_bytes(C.byref(self._w), B, L, n_label_rows), device=dev, dtype=torch.uint8)
        loss = torch.zeros(1, device=dev, dtype=F32)
        nll = torch.empty(max(n_label_rows, 1), device=dev, dtype=F32)
        logits = torch.empty((B * L, self.vocab_pad), device=dev, dtype=BF16) if want_logits else None
        if seg is not None and (seg.dtype != torch.int32 or seg.numel() != 2 * B * L or not seg.is_contiguous()):
            raise ValueError(f"seg must be a contiguous int32 [2, {B * L}] segment table; got {seg.dtype} {tuple(seg.shape)}")
        obj, ce = None, None
        if eps > 0.0 or zc > 0.0:
            obj = torch.zeros(max(n_label_rows, 1), device=dev, dtype=F32)
            ce = _lib.CeOptions(eps=eps, zc=zc, obj=obj.data_ptr())
        _lm_call("forward", (C.byref(self._w), ptr(input_ids), ptr(src_row), ptr(audio), ptr(kmask), ptr(pos)), seg,
                 (B, L, ptr(label_rows), ptr(label_targets), n_label_rows, loss_scale, ptr(loss), ptr(nll), ptr(logits), ptr(tape),
                  ptr(ws), ws.numel()), _lora_drop_desc(lora_dropout), ce)
        # ``modes``: the tape's residual-stream rows are in the storage dtype this handle carries NOW; the backward must read them as
        # that even if the owner flips ``res_f32`` in between
        ctx = dict(tape=tape, ws=ws, B=B, L=L, src_row=src_row, kmask=kmask, pos=pos, label_rows=label_rows,
                   n_label_rows=n_label_rows, ids=input_ids, lora_dropout=lora_dropout, seg=seg,
                   modes=(bool(self._w.res_f32), bool(self._w.dx_f32)))
        if obj is not None:
            ctx["obj"] = obj
        return loss, nll, logits, ctx

    def backward_from_ctx(self, ctx, n_audio_rows, want_d_embeds=False, want_d_audio=True):
        """-> (d_audio f32 [n_audio_rows, D] or None, d_embeds f32 [B*L, D] or None, trainable-LM gradients or None) for
        d(loss) = 1.  The third item is the list of adapter gradients (order of ``lora_parameters()``) with LoRA, the list
        of weight gradients (order of ``ft_parameters()``) with a trainable base LM -- or ``[None] * 10`` when
        ``accumulate_into_grad`` is set and they were added straight into ``Parameter.grad``."""
        D, dev = self.config.hidden_size, self.device_
        d_audio = torch.empty((n_audio_rows, D), device=dev, dtype=F32) if want_d_audio else None
        d_emb = torch.empty((ctx["B"] * ctx["L"], D), device=dev, dtype=F32) if want_d_embeds else None
        lg, lg_arr, wg, keep = None, None, None, None
        nl = self.config.num_hidden_layers
        if self.lora_rank:
            self._bind_lora()
            lg = [torch.empty_like(p) for p in self.lora_parameters()]
            lg_arr = (_lib.LmLoraGrads * nl)()
            k = 0
            for g, _ in LORA_GROUPS:
                for ab in ("la", "lb"):
                    step = lg[k][0].numel() * 4
                    for i in range(nl):
                        setattr(lg_arr[i], f"d{ab}_{g}", lg[k].data_ptr() + i * step)
                    k += 1
        if self.train_base:
            ps = self.ft_parameters()
            direct = self.accumulate_into_grad and all(p.grad is not None and p.grad.is_contiguous() for p in ps)
            bufs = [p.grad for p in ps] if direct else [torch.zeros_like(p) for p in ps]
            arr = (_lib.LmLayerWgrads * nl)()
            for (kind, _), g in zip(self.FT_KINDS, bufs):
                field = {"wqkv": "dwqkv", "wo": "dwo", "wgu": "dwgu", "wd": "dwd", "ln_in_w": "dln_in", "ln_post_w": "dln_post",
                         "qn_w": "dqn", "kn_w": "dkn"}[kind]
                step = g[0].numel() * 4
                for i in range(nl):
                    setattr(arr[i], field, g.data_ptr() + i * step)
            wg = _lib.LmWgrads(layers=C.cast(arr, C.POINTER(_lib.LmLayerWgrads)), dnorm=bufs[8].data_ptr(), dembed=bufs[9].data_ptr())
            keep = (arr, bufs)
            lg = [None] * len(ps) if direct else bufs
        w = self._w
        if ctx["modes"] != (bool(w.res_f32), bool(w.dx_f32)):
            w = _lib.LmWeights.from_buffer_copy(self._w)          # same pointers, the modes the forward ran in
            w.res_f32, w.dx_f32 = (int(v) for v in ctx["modes"])
        # ... with the segment table and the dropout descriptor its forward ran with
        _lm_call("backward", (C.byref(w), ptr(ctx["src_row"]), ptr(ctx["kmask"]), ptr(ctx["pos"])), ctx["seg"],
                 (ctx["B"], ctx["L"], ptr(ctx["label_rows"]), ctx["n_label_rows"], ptr(d_audio), n_audio_rows, ptr(d_emb), lg_arr,
                  None if wg is None else C.byref(wg), ptr(ctx["ids"]), ptr(ctx["tape"]), ptr(ctx["ws"]), ctx["ws"].numel()),
                 _lora_drop_desc(ctx["lora_dropout"]))
        del keep
        return d_audio, d_emb, lg

    # ------------------------------------------------------------------ decoding: the drivers of decoding.py, bound as methods (lm = self)
    greedy_decode, greedy_decode_iter = decoding.greedy_decode, decoding.greedy_decode_iter
    beam_decode, score_candidates = decoding.beam_decode, decoding.score_candidates


def _lora_drop_desc(d):
    """(p, seed, offset) -> ta_lora_dropout, or None when dropout is off (None or p == 0: the plain entry points run)."""
    if d is None or not float(d[0]) > 0.0:
        return None
    return _lib.LoraDropout(p=float(d[0]), seed=int(d[1]) & 0xFFFFFFFFFFFFFFFF, offset=int(d[2]) & 0xFFFFFFFFFFFFFFFF)


def check_loss_options(label_smoothing, z_loss):
    """(label_smoothing, z_loss) as floats; ValueError outside 0 <= label_smoothing < 1, z_loss >= 0 (the library's TA_ERR_ARG)."""
    eps, zc = float(label_smoothing or 0.0), float(z_loss or 0.0)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1); got {label_smoothing}")
    if not zc >= 0.0:
        raise ValueError(f"z_loss must be >= 0; got {z_loss}")
    return eps, zc


_LM_ENTRY = {"forward": ("ta_lm_forward_loss", "ta_lm_forward_loss_ex", "ta_lm_forward_loss_seg"),
             "backward": ("ta_lm_backward", "ta_lm_backward_ex", "ta_lm_backward_seg")}


def _lm_call(direction, head, seg, tail, drop, ce=None):
    """Run the LM entry point of ``direction`` that (seg, drop) select: the plain one with neither, _ex with a dropout descriptor only,
    _seg with a segment table (its descriptor may be NULL).  All three take ``head`` (... pos), then the table, then ``tail``
    (B ... ws_bytes), then the descriptor, then the stream.  ``ce`` (forward only): a ta_ce_options selects ta_lm_forward_loss_opt,
    the _seg arguments (table and descriptor may be NULL) followed by the options."""
    plain, ex, packed = _LM_ENTRY[direction]
    d = None if drop is None else C.byref(drop)
    if ce is not None:
        name, args = "ta_lm_forward_loss_opt", (*head, ptr(seg), *tail, d, C.byref(ce), stream())
    elif seg is not None:
        name, args = packed, (*head, ptr(seg), *tail, d, stream())
    elif drop is not None:
        name, args = ex, (*head, *tail, d, stream())
    else:
        name, args = plain, (*head, *tail, stream())
    _lib.check(getattr(_lib.lib(), name)(*args), name)


class FrozenLMLoss:
    """loss = CE(frozen_LM(embed(ids) with <audio> rows := audio_embeds)) through ``torch.ops.ta355.lm_forward_loss``
    (torch_ops.py); grad flows to audio_embeds and to the trainable LM tensors passed as trailing inputs -- the LoRA masters
    (``*lm.lora_parameters()``) or, with a trainable base LM, its fp32 masters (``*lm.ft_parameters()``).

    One operator pair (``lm_forward_loss`` / ``lm_backward``) serves every configuration: ``seg`` (the table of
    ``ops.segment_table``) selects packed rows, and the (p, seed, offset) of ``lm.next_lora_dropout()`` selects LoRA dropout, p = 0
    being "off".  The autograd node keeps both, and the two residual-stream modes the forward ran in, for ITS backward.
    ``label_smoothing`` / ``z_loss`` (``forward_loss``) change the loss and the dlogits the forward leaves on the tape; the backward
    is the same call.

    accumulate_into_grad (full decoder fine-tuning under ASRTrainer): the kernels add the LM's weight gradients straight
    into the trainer's flat buffer, so d(loss) cannot be applied to them afterwards.  ASRTrainer is the only caller that
    sets the flag and it always back-propagates the CE with d(loss) == 1 (the auxiliary term is added outside this node,
    the token normalisation happens in the optimizer kernel); any other use must leave it off."""

    @staticmethod
    def apply(audio_embeds, lm, input_ids, src_row, kmask, label_rows, label_targets, n_label_rows, loss_scale,
              want_logits, *trainable, pos=None, seg=None, label_smoothing=0.0, z_loss=0.0):
        from . import torch_ops
        # training forwards of a p > 0 model only: a fresh Philox offset each; lora_p = 0 is "no dropout"
        drop = lm.next_lora_dropout() or (0.0, 0, 0)
        # the loss options trail the operator's arguments; left out at 0, the call dispatches as it did before they existed
        eps, zc = check_loss_options(label_smoothing, z_loss)
        opts = (eps, zc) if (eps > 0.0 or zc > 0.0) else ()
        loss, nll, logits, _tape, _ws = torch.ops.ta355.lm_forward_loss(
            audio_embeds, list(trainable), torch_ops.register_module(lm), input_ids, src_row, kmask, label_rows, label_targets,
            int(n_label_rows), float(loss_scale), bool(want_logits), pos, seg, *drop, *opts)
        # a fresh tensor: the outputs of a multi-output custom op may not be modified in place, and HF Trainer does
        # `loss *= ...` on what the model returns (TF:trainer.py compute_loss)
        return loss.clone(), nll, logits
