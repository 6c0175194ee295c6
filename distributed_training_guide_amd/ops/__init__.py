"""HIP-kernel-backed ops (GPU) with eager fp32 references (CPU/tests)."""
from .adamw import FusedAdamW, join_master, split_master
from .attention import flash_attention
from .cross_entropy import causal_lm_loss, sharded_causal_lm_loss
from .doc_mask import (DocBounds, doc_bounds, doc_start_from_ids,
                       validate_doc_start)
from .fp8_linear import (Fp8Linear, convert_linears_to_fp8, fp8_linear,
                         fp8_quantize)
from .fused_linear_ce import fused_causal_lm_loss
from .grad_clip import clip_grad_norm_, grad_sq_sum
from .layernorm import LayerNorm, gelu
from .qk_norm import qkv_norm_rope
from .rmsnorm import RMSNorm, rmsnorm
from .rope import qkv_rope, rope
from .swiglu import silu_mul

__all__ = [
    "FusedAdamW",
    "split_master",
    "join_master",
    "flash_attention",
    "causal_lm_loss",
    "sharded_causal_lm_loss",
    "DocBounds",
    "doc_bounds",
    "doc_start_from_ids",
    "validate_doc_start",
    "Fp8Linear",
    "convert_linears_to_fp8",
    "fp8_linear",
    "fp8_quantize",
    "fused_causal_lm_loss",
    "clip_grad_norm_",
    "grad_sq_sum",
    "LayerNorm",
    "gelu",
    "RMSNorm",
    "rmsnorm",
    "qkv_norm_rope",
    "qkv_rope",
    "rope",
    "silu_mul",
]
