"""Llama-family causal LM built directly on the gfx950 HIP ops.

Config-compatible shapes with transformers' Llama (the reference builds its
models via AutoModelForCausalLM.from_config,
/root/reference/01-single-gpu/train_llm.py:47-49) but implemented natively:
RMSNorm / RoPE / flash attention / SwiGLU / fused CE are this repo's HIP
kernels; the projections are plain GEMMs (hipBLASLt via torch.linear).

MI355X-first choices:
  * BSHD activations everywhere — q/k/v go from the packed qkv GEMM into the
    attention kernel without a single transpose.
  * qkv packed as ONE GEMM (q | k | v segments), gate+up packed as ONE GEMM
    (halved launch count; the TP layer shards these segment-aware).
  * vocab padded to a multiple of 64 (GEMM-friendly; CE kernel needs /8).
  * meta-device init + init_weights()/reset_parameters() flow supported for
    the FSDP chapters (reference 04:74-95, 06:123-125).
"""
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from ..ops import (RMSNorm, causal_lm_loss, doc_bounds, flash_attention,
                   moe_mlp, qkv_norm_rope, qkv_rope, silu_mul)
from ..ops.embedding import Embedding
from ..ops.fp8_linear import fp8_swiglu_linear
from ..ops.fused_linear_ce import fused_causal_lm_loss
from ..ops.rmsnorm import add_rmsnorm


def pad_vocab(v: int, multiple: int = 64) -> int:
    return (v + multiple - 1) // multiple * multiple


@dataclass
class LlamaConfig:
    vocab_size: int = 32000
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 32
    max_position_embeddings: int = 4096
    rope_theta: float = 10000.0
    rms_norm_eps: float = 1e-5
    initializer_range: float = 0.02
    tie_word_embeddings: bool = False
    model_type: str = field(default="llama")
    # QK-norm (Qwen3, OLMo-2, Gemma-3): an RMSNorm with a learned [head_dim]
    # weight on every q and k head, after the projection and before RoPE
    qk_norm: bool = False
    # explicit head dim for models that decouple it from hidden / heads
    # (Qwen3 uses 128 throughout); None = hidden_size // num_attention_heads
    head_dim_override: int | None = None
    # mixture of experts (Qwen3-MoE): num_experts > 0 replaces every layer's
    # dense MLP by num_experts SwiGLU experts of moe_intermediate_size, each
    # token routed to num_experts_per_tok of them; norm_topk_prob
    # renormalises the router's softmax over the selected experts
    num_experts: int = 0
    num_experts_per_tok: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = True
    # router regularisers (ops/moe.py): the loss gains
    # router_aux_loss_coef * mean over layers of the load-balancing loss (HF
    # trains Qwen3-MoE with 0.001) and router_z_loss_coef * mean over layers
    # of the router z-loss.  With both 0 the router is called without them.
    router_aux_loss_coef: float = 0.0
    router_z_loss_coef: float = 0.0
    # the expert GEMMs (ops/moe.py expert_mm): "torch" is torch's grouped
    # GEMM, "hip" the hand-written grouped GEMMs of _hip/moe_gemm.hip,
    # "hip-gather" those without the expert-sorted copy of the tokens
    # (_hip/moe_gemm_gather.hip), "hip-fused" those with the weighted SwiGLU
    # in the GEMMs' epilogues (_hip/moe_gemm_swiglu.hip)
    expert_gemm: str = "torch"

    @property
    def router_losses(self) -> bool:
        return self.router_aux_loss_coef != 0 or self.router_z_loss_coef != 0

    @property
    def head_dim(self) -> int:
        if self.head_dim_override is not None:
            return self.head_dim_override
        return self.hidden_size // self.num_attention_heads

    @property
    def padded_vocab_size(self) -> int:
        return pad_vocab(self.vocab_size)

    def num_parameters(self) -> int:
        h, i, v = self.hidden_size, self.intermediate_size, self.padded_vocab_size
        d = self.head_dim
        hq = self.num_attention_heads
        # o_proj is [h, Hq*d]: h*h unless the head dim is set explicitly
        attn = h * (hq + 2 * self.num_key_value_heads) * d + hq * d * h
        if self.qk_norm:
            attn += 2 * d
        mlp = 3 * h * i
        if self.num_experts > 0:  # the experts and the router
            mlp = self.num_experts * (3 * h * self.moe_intermediate_size + h)
        per_layer = attn + mlp + 2 * h
        embed = v * h * (1 if self.tie_word_embeddings else 2)
        return per_layer * self.num_hidden_layers + embed + h


@dataclass
class CausalLMOutput:
    loss: torch.Tensor | None = None
    logits: torch.Tensor | None = None
    # means over the MoE layers, set when the config asks for router losses
    router_aux_loss: torch.Tensor | None = None
    router_z_loss: torch.Tensor | None = None


class LlamaAttention(nn.Module):
    def __init__(self, config: LlamaConfig, device=None, dtype=None):
        super().__init__()
        self.config = config
        h = config.hidden_size
        d = config.head_dim
        self.num_heads = config.num_attention_heads
        self.num_kv_heads = config.num_key_value_heads
        self.head_dim = d
        # packed q|k|v projection — one GEMM
        self.qkv_proj = nn.Linear(
            h, (self.num_heads + 2 * self.num_kv_heads) * d, bias=False,
            device=device, dtype=dtype)
        self.o_proj = nn.Linear(self.num_heads * d, h, bias=False,
                                device=device, dtype=dtype)
        if config.qk_norm:
            # weight holders (HF names self_attn.q_norm / k_norm): forward
            # hands their weights to the fused split + norm + RoPE kernel
            self.q_norm = RMSNorm(d, config.rms_norm_eps, device, dtype)
            self.k_norm = RMSNorm(d, config.rms_norm_eps, device, dtype)

    def forward(self, x, position_ids=None, doc=None):
        B, S, _ = x.shape
        d = self.head_dim
        qkv = self.qkv_proj(x)
        if self.config.qk_norm:
            # fused split + per-head RMSNorm of q and k + RoPE
            q, k, v = qkv_norm_rope(
                qkv, self.q_norm.weight, self.k_norm.weight, self.num_heads,
                self.num_kv_heads, d, self.q_norm.eps,
                self.config.rope_theta, positions=position_ids,
                max_pos=self.config.max_position_embeddings)
        else:
            # fused split + RoPE: one pass, no intermediate copies, backward
            # writes dqkv directly (no grad cat)
            q, k, v = qkv_rope(qkv, self.num_heads, self.num_kv_heads, d,
                               self.config.rope_theta, positions=position_ids,
                               max_pos=self.config.max_position_embeddings)
        o = flash_attention(q, k, v, doc=doc)
        return self.o_proj(o.reshape(B, S, self.num_heads * d))


class LlamaMLP(nn.Module):
    def __init__(self, config: LlamaConfig, device=None, dtype=None):
        super().__init__()
        h, i = config.hidden_size, config.intermediate_size
        # packed gate|up projection — one GEMM
        self.gate_up_proj = nn.Linear(h, 2 * i, bias=False, device=device,
                                      dtype=dtype)
        self.down_proj = nn.Linear(i, h, bias=False, device=device,
                                   dtype=dtype)

    def forward(self, x):
        # a down projection under FP8 delayed scaling takes SwiGLU's result
        # as e4m3 straight from the kernel (ops/fp8_linear.py)
        state = getattr(self.down_proj, "fp8_state", None)
        if state is not None:
            return fp8_swiglu_linear(self.gate_up_proj(x),
                                     self.down_proj.weight, state)
        return self.down_proj(silu_mul(self.gate_up_proj(x)))


class LlamaMoE(nn.Module):
    """Mixture-of-experts feed-forward (ops/moe.py): a bias-free router and
    the experts' weights as two 3-D parameters, gate|up packed per expert
    like LlamaMLP's.  The router's weight goes to the op directly and
    convert_linears_to_fp8 skips modules named `router`, so the router GEMM
    is bf16 and is reported as such."""

    def __init__(self, config: LlamaConfig, device=None, dtype=None):
        super().__init__()
        h, i, e = (config.hidden_size, config.moe_intermediate_size,
                   config.num_experts)
        if not 1 <= config.num_experts_per_tok <= e:
            raise ValueError(
                f"num_experts_per_tok must be in [1, {e}], got "
                f"{config.num_experts_per_tok}")
        self.top_k = config.num_experts_per_tok
        self.norm_topk_prob = config.norm_topk_prob
        self.expert_gemm = config.expert_gemm
        # (aux, z) of the latest forward.  One attribute, overwritten every
        # forward: the model reads it right after the layer loop, so the
        # loss is built on the graph of that forward, and a checkpoint
        # recompute during backward only replaces what was already used.
        self.router_losses = config.router_losses
        self.aux_losses = None
        self.router = nn.Linear(h, e, bias=False, device=device, dtype=dtype)
        self.gate_up_proj = nn.Parameter(
            torch.empty(e, 2 * i, h, device=device, dtype=dtype))
        self.down_proj = nn.Parameter(
            torch.empty(e, h, i, device=device, dtype=dtype))

    def forward(self, x):
        tokens = x.reshape(-1, x.shape[-1])
        if self.router_losses:
            y, *self.aux_losses = moe_mlp(
                tokens, self.router.weight, self.gate_up_proj,
                self.down_proj, self.top_k, self.norm_topk_prob, aux=True,
                expert_gemm=self.expert_gemm)
        else:
            y = moe_mlp(tokens, self.router.weight, self.gate_up_proj,
                        self.down_proj, self.top_k, self.norm_topk_prob,
                        expert_gemm=self.expert_gemm)
        return y.view(x.shape)


class LlamaDecoderLayer(nn.Module):
    def __init__(self, config: LlamaConfig, device=None, dtype=None):
        super().__init__()
        self.input_layernorm = RMSNorm(config.hidden_size,
                                       config.rms_norm_eps, device, dtype)
        self.self_attn = LlamaAttention(config, device, dtype)
        self.post_attention_layernorm = RMSNorm(
            config.hidden_size, config.rms_norm_eps, device, dtype)
        mlp_cls = LlamaMoE if config.num_experts > 0 else LlamaMLP
        self.mlp = mlp_cls(config, device, dtype)

    def forward(self, x, position_ids=None, residual=None, doc=None):
        """Two call forms (both via __call__ so FSDP/checkpoint hooks fire):
        - forward(x): the reference chain x + attn(norm(x)) + mlp(...).
        - forward(delta, residual=res): fused (delta, residual) threading —
          each residual add is fused into the next RMSNorm kernel; returns
          (new_delta, new_residual), equivalent to forward(res + delta).
        doc: the model's DocBounds (document-masked attention) or None.
        """
        if residual is None:
            x = x + self.self_attn(self.input_layernorm(x), position_ids,
                                   doc=doc)
            x = x + self.mlp(self.post_attention_layernorm(x))
            return x
        normed, residual = add_rmsnorm(residual, x,
                                       self.input_layernorm.weight,
                                       self.input_layernorm.eps)
        a = self.self_attn(normed, position_ids, doc=doc)
        normed, residual = add_rmsnorm(residual, a,
                                       self.post_attention_layernorm.weight,
                                       self.post_attention_layernorm.eps)
        return self.mlp(normed), residual


class LlamaForCausalLM(nn.Module):
    def __init__(self, config: LlamaConfig, device=None, dtype=None):
        super().__init__()
        self.config = config
        v = config.padded_vocab_size
        h = config.hidden_size
        self.embed_tokens = Embedding(v, h, device=device, dtype=dtype)
        self.layers = nn.ModuleList(
            LlamaDecoderLayer(config, device, dtype)
            for _ in range(config.num_hidden_layers))
        self.norm = RMSNorm(h, config.rms_norm_eps, device, dtype)
        self.lm_head = nn.Linear(h, v, bias=False, device=device, dtype=dtype)
        if config.tie_word_embeddings:
            self.lm_head.weight = self.embed_tokens.weight
        self.init_weights()

    # ---- init flow (meta-device friendly; reference 04:74-95, 06:123-125) --
    def init_weights(self):
        std = self.config.initializer_range
        with torch.no_grad():
            for m in self.modules():
                self._reset_module(m, std)

    def reset_param_by_name(self, name: str, tensor: torch.Tensor):
        """Initialize one (materialized) parameter by its qualified name —
        used by the FSDP engine's unit-by-unit meta materialization
        (reference flow 04:74-95)."""
        std = self.config.initializer_range
        with torch.no_grad():
            if "layernorm" in name or name.startswith("norm.") \
                    or ".q_norm." in name or ".k_norm." in name:
                tensor.fill_(1.0)
            elif name.endswith(".bias"):
                tensor.zero_()
            else:
                tensor.normal_(0.0, std)

    @staticmethod
    def _reset_module(m, std):
        if isinstance(m, (nn.Linear, nn.Embedding, Embedding)):
            if not m.weight.is_meta:
                m.weight.normal_(0.0, std)
            if isinstance(m, nn.Linear) and m.bias is not None \
                    and not m.bias.is_meta:
                m.bias.zero_()
        elif isinstance(m, RMSNorm):
            m.reset_parameters()
        elif isinstance(m, LlamaMoE):  # the router is an nn.Linear (above)
            for p in (m.gate_up_proj, m.down_proj):
                if not p.is_meta:
                    p.normal_(0.0, std)

    def forward(self, input_ids, labels=None, attention_mask=None,
                position_ids=None, doc_start=None, **_):
        """doc_start (int32 [B,S], ops/doc_mask.py) confines attention to
        each token's own document of a packed row; without it attention is
        causal over the whole row.  Positions are NOT reset per document:
        RoPE scores depend only on i - j, so attention inside a document is
        the same whether its positions start at 0 or at its offset in the
        row."""
        # attention_mask accepted for API parity (reference data pipeline
        # emits it, 01:69); attention is always causal over packed rows.
        if position_ids is not None and position_ids.dim() == 2:
            position_ids = position_ids[0]
        # both mask tables once per forward; every layer (and every
        # checkpoint recompute) gets this same object
        doc = None if doc_start is None else doc_bounds(doc_start)
        x = self.embed_tokens(input_ids)
        if x.is_cuda:
            # fused (delta, residual) path: every residual add is fused
            # into the next RMSNorm kernel (norm.hip). Every layer
            # is entered through __call__ so FSDP / activation-checkpoint
            # hooks fire; the zero first delta costs one extra H-read.
            residual = x
            delta = torch.zeros_like(x)
            for layer in self.layers:
                delta, residual = layer(delta, position_ids,
                                        residual=residual, doc=doc)
            x, _ = add_rmsnorm(residual, delta, self.norm.weight,
                               self.norm.eps)
        else:
            for layer in self.layers:
                x = layer(x, position_ids, doc=doc)
            x = self.norm(x)
        aux = z = None
        if self.config.router_losses and self.config.num_experts > 0:
            # each layer's (aux, z) from the forward that just ran, averaged
            per_layer = [layer.mlp.aux_losses for layer in self.layers]
            aux = torch.stack([a for a, _ in per_layer]).mean()
            z = torch.stack([b for _, b in per_layer]).mean()
        if labels is not None and x.is_cuda:
            # chunked fused projection+CE: the [B,S,V] logits (+grad) are
            # never materialized (ops/fused_linear_ce.py) — logits=None,
            # like the reference's loss-only training consumers (02:149-163
            # only reads outputs.loss)
            loss = fused_causal_lm_loss(x, self.lm_head.weight, labels)
            return CausalLMOutput(self._with_router_losses(loss, aux, z),
                                  None, aux, z)
        logits = self.lm_head(x)
        loss = None
        if labels is not None:
            loss = self._with_router_losses(causal_lm_loss(logits, labels),
                                            aux, z)
        return CausalLMOutput(loss, logits, aux, z)

    def _with_router_losses(self, loss, aux, z):
        if aux is None:
            return loss
        return loss + self.config.router_aux_loss_coef * aux \
            + self.config.router_z_loss_coef * z
