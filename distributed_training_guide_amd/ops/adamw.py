"""Fused multi-tensor AdamW on the gfx950 HIP kernel (adamw.hip).

Drop-in for the reference's torch.optim.AdamW(fused=True)
(/root/reference/01-single-gpu/train_llm.py:73 and every later chapter).
One kernel launch updates every chunk of every parameter; fp32 moments;
bf16 or fp32 params; bf16 or fp32 grads (fp32 under FSDP's reduce_dtype).
Chunk descriptors are cached and rebuilt only when tensor addresses change.
Optional global-norm gradient clipping (max_grad_norm) is fused into the
update: grad_norm.hip computes the device-resident squared norm, the clipped
kernel variant scales g while loading it.

CPU path (cpu-offload chapter, unit tests): eager fp32 math with identical
update order/semantics.

Master weights (master_weights=True), 16-bit extended.  A bf16 parameter
keeps 8 significant bits, so an update below half an ulp is rounded away
entirely (at lr 3e-5 from |w| ~ 2^-6 on).  With the option on, every bf16
parameter gets an int16 companion, state["master_lo"], and the pair holds an
fp32 master exactly.  For the master's fp32 bit pattern u, in 32-bit
wrap-around arithmetic:

    hi = (u + 0x8000) >> 16          the bf16 parameter's bits
    lo = int16(u - (hi << 16))       the companion
    u  = (hi << 16) + sext(lo)       reconstruction

hi is u rounded to nearest on the magnitude with ties AWAY from zero; it is
not the ties-to-even of `.bfloat16()`, whose remainder would need +-0x8000
and not fit 16 bits.  The two differ at exact ties only.  A NaN master is
stored as (0x7FC0, 0): the wrapped hi of a NaN can be +-0 or +-inf, and the
model, which reads the bf16 tensor alone, must see a NaN.  A finite master
above the largest finite bf16 shows as bf16 inf while the pair stays finite.
The model keeps reading the bf16 tensor it reads today; there is no extra
copy or cast, the update kernel streams 26 B per element for 22.
split_master / join_master below are this rule (adamw.hip has the same one
as master_split / master_join).
"""
import logging

import torch

from .._ext import ext

LOGGER = logging.getLogger(__name__)

CHUNK = 262144  # elements per descriptor chunk; must match adamw.hip

_QNAN_BF16 = 0x7FC0


def split_master(fp32):
    """fp32 master -> (bf16 parameter, int16 companion); see the module
    docstring.  Round to nearest, ties away from zero; NaN -> (0x7FC0, 0).
    Pure torch integer ops, any device."""
    if fp32.dtype != torch.float32:
        raise TypeError(f"split_master expects float32, got {fp32.dtype}")
    u = fp32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    hi = ((u + 0x8000) & 0xFFFFFFFF) >> 16
    lo = (u - (hi << 16)) & 0xFFFFFFFF            # mod 2^32 ...
    lo = ((lo + 0x8000) & 0xFFFFFFFF) - 0x8000    # ... as a signed value
    nan = torch.isnan(fp32)
    hi = torch.where(nan, torch.full_like(hi, _QNAN_BF16), hi)
    lo = torch.where(nan, torch.zeros_like(lo), lo)
    hi = (hi ^ 0x8000) - 0x8000                   # bits as a signed int16
    return (hi.to(torch.int16).view(torch.bfloat16).view(fp32.shape),
            lo.to(torch.int16).view(fp32.shape))


def join_master(bf16, lo):
    """(bf16 parameter, int16 companion) -> the fp32 master, exactly."""
    if bf16.dtype != torch.bfloat16 or lo.dtype != torch.int16:
        raise TypeError("join_master expects (bfloat16, int16), got "
                        f"({bf16.dtype}, {lo.dtype})")
    hi = bf16.contiguous().view(torch.int16).to(torch.int64)
    u = (hi << 16) + lo.to(torch.int64)
    u = ((u + 0x80000000) & 0xFFFFFFFF) - 0x80000000  # wrap to int32
    return u.to(torch.int32).view(torch.float32).view(bf16.shape)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, max_grad_norm=0.0, grad_norm_parts=None,
                 master_weights=False):
        """max_grad_norm > 0 turns on global-norm gradient clipping fused
        into the update (0 = off): one extra read-only pass computes the
        squared grad sum over ALL param groups, the scale
        min(1, max_grad_norm / (norm + 1e-6)) multiplies g as it is loaded —
        `p.grad` is left untouched and the host never waits.
        `grad_norm_parts` is a list of (params, process_group_or_None) that
        says how the global norm is assembled on a sharded engine (see
        ops/grad_clip.py); its params need not be this optimizer's own.
        Default: this optimizer's params, complete on this rank.

        master_weights=True keeps an fp32 master of every bf16 parameter as
        the pair (parameter, state["master_lo"]) described in the module
        docstring: +2 B per bf16 parameter, zeros at first touch, so the
        master starts as the exact widening of the bf16 value.  fp32
        parameters already are their own master and get no companion.
        `lo` belongs to the value the optimizer last wrote: after
        parameters are overwritten from outside (weights loaded, a
        broadcast), call reset_master()."""
        if max_grad_norm < 0:
            raise ValueError(f"invalid max_grad_norm {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay, step=0,
                        max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self._desc_cache = {}  # group idx -> (key, desc, nchunks, lo_tab)
        self.grad_norm_parts = None
        if grad_norm_parts is not None:
            self.grad_norm_parts = [(list(ps), group)
                                    for ps, group in grad_norm_parts]
        # pre-clip global grad norm of the last clipped step (0-dim fp32
        # device tensor); None until then
        self.last_grad_norm = None
        self._norm_tables = None
        self.master_weights = bool(master_weights)

    def _get_state(self, p):
        state = self.state[p]
        if "exp_avg" not in state:
            state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
        if (self.master_weights and p.dtype == torch.bfloat16
                and "master_lo" not in state):
            state["master_lo"] = torch.zeros_like(
                p, dtype=torch.int16, memory_format=torch.contiguous_format)
        return state

    # ---------------- master weights ----------------
    def master_param(self, p):
        """The fp32 master of `p`: join_master(p, master_lo) for a bf16
        parameter of a master-weight optimizer, p.float() otherwise (an
        fp32 parameter, the option off, or no step taken yet)."""
        lo = self.state.get(p, {}).get("master_lo") \
            if self.master_weights else None
        if lo is None or p.dtype != torch.bfloat16:
            return p.detach().float()
        return join_master(p.detach(), lo)

    @torch.no_grad()
    def reset_master(self):
        """Zero every companion: the master becomes the exact widening of
        the current bf16 values.  Call it after parameters were overwritten
        from outside the optimizer; a stale `lo` would otherwise be added
        to a value it does not belong to."""
        for st in self.state.values():
            if "master_lo" in st:
                st["master_lo"].zero_()

    def master_summary(self):
        """(parameters that carry a companion, their elements, extra bytes)
        for this optimizer's parameters."""
        ps = [p for g in self.param_groups for p in g["params"]
              if self.master_weights and p.dtype == torch.bfloat16]
        n = sum(p.numel() for p in ps)
        return len(ps), n, 2 * n

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sq_total = None
        if any(g.get("max_grad_norm", 0.0) > 0 for g in self.param_groups):
            sq_total = self._global_sq_sum()
            self.last_grad_norm = sq_total.sqrt()
        for gi, group in enumerate(self.param_groups):
            group["step"] += 1
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            clip = sq_total if group.get("max_grad_norm", 0.0) > 0 else None
            if params[0].is_cuda:
                self._step_hip(gi, group, params, clip)
            else:
                self._step_eager(group, params, clip)
        return loss

    def _global_sq_sum(self):
        """Squared global grad norm over every param group (or over
        grad_norm_parts), all-reduced per part; stays on the device."""
        from . import grad_clip

        if self._norm_tables is None:
            self._norm_tables = grad_clip._GradTable()
        parts = self.grad_norm_parts
        if parts is None:
            parts = [([p for g in self.param_groups for p in g["params"]],
                      None)]
        return grad_clip.total_sq_sum(parts, self._norm_tables)

    # ---------------- HIP multi-tensor path ----------------
    def _step_hip(self, gi, group, params, sq_total=None):
        master = self.master_weights and any(
            p.dtype == torch.bfloat16 for p in params)
        if master:
            key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel(),
                         self._get_state(p)["master_lo"].data_ptr()
                         if p.dtype == torch.bfloat16 else 0)
                        for p in params)
        else:
            key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel())
                        for p in params)
        cached = self._desc_cache.get(gi)
        if cached is None or cached[0] != key:
            # grad addresses change whenever zero_grad(set_to_none=True)
            # lets autograd re-allocate, so this rebuild can run EVERY
            # step — build the [nchunks, 7] descriptor table with
            # vectorized numpy per param (a Python list-of-lists +
            # torch.tensor took ~10 ms for an 8B model's ~30k chunks,
            # a visible GPU idle bubble before the update kernel).
            import numpy as np

            blocks, lo_blocks = [], []
            for p in params:
                g = p.grad
                if not g.is_contiguous():
                    raise RuntimeError("FusedAdamW requires contiguous grads")
                st = self._get_state(p)
                n = p.numel()
                p_bf = 1 if p.dtype == torch.bfloat16 else 0
                g_bf = 1 if g.dtype == torch.bfloat16 else 0
                if p.dtype not in (torch.bfloat16, torch.float32):
                    raise RuntimeError(f"unsupported param dtype {p.dtype}")
                esz_p = 2 if p_bf else 4
                esz_g = 2 if g_bf else 4
                offs = np.arange(0, n, CHUNK, dtype=np.int64)
                rows = np.empty((len(offs), 7), dtype=np.int64)
                rows[:, 0] = p.data_ptr() + offs * esz_p
                rows[:, 1] = g.data_ptr() + offs * esz_g
                rows[:, 2] = st["exp_avg"].data_ptr() + offs * 4
                rows[:, 3] = st["exp_avg_sq"].data_ptr() + offs * 4
                rows[:, 4] = np.minimum(CHUNK, n - offs)
                rows[:, 5] = p_bf
                rows[:, 6] = g_bf
                blocks.append(rows)
                if master:
                    # parallel [nchunks] table of companion pointers; the
                    # 7-column table is shared with grad_norm.hip and stays
                    if p_bf:
                        lo = st["master_lo"]
                        if not lo.is_contiguous() or lo.shape != p.shape \
                                or lo.device != p.device:
                            raise RuntimeError(
                                "master_lo must be a contiguous int16 "
                                "tensor of the parameter's shape and device")
                        lo_blocks.append(lo.data_ptr() + offs * 2)
                    else:
                        lo_blocks.append(np.zeros(len(offs), dtype=np.int64))
            table = np.concatenate(blocks)
            desc = torch.from_numpy(table).to(params[0].device,
                                              non_blocking=True)
            lo_tab = None
            if master:
                lo_tab = torch.from_numpy(np.concatenate(lo_blocks)).to(
                    params[0].device, non_blocking=True)
            self._desc_cache[gi] = (key, desc, len(table), lo_tab)
        _, desc, nchunks, lo_tab = self._desc_cache[gi]
        b1, b2 = group["betas"]
        if lo_tab is not None:
            ext().adamw_master_step(
                desc, lo_tab, nchunks, group["lr"], b1, b2, group["eps"],
                group["weight_decay"], group["step"],
                None if sq_total is None
                else sq_total.to(desc.device).reshape(1),
                group["max_grad_norm"])
        elif sq_total is None:
            ext().adamw_step(desc, nchunks, group["lr"], b1, b2, group["eps"],
                             group["weight_decay"], group["step"])
        else:
            ext().adamw_step_clipped(
                desc, nchunks, group["lr"], b1, b2, group["eps"],
                group["weight_decay"], group["step"],
                sq_total.to(desc.device).reshape(1), group["max_grad_norm"])

    # ---------------- eager path (CPU / reference) ----------------
    def _step_eager(self, group, params, sq_total=None):
        b1, b2 = group["betas"]
        t = group["step"]
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        coef = None
        if sq_total is not None:
            from .grad_clip import clip_coef

            coef = clip_coef(sq_total.to(params[0].device),
                             group["max_grad_norm"])
        for p in params:
            st = self._get_state(p)
            g = p.grad.float()
            if coef is not None:
                g = g * coef  # scaled copy: p.grad stays untouched
            m, v = st["exp_avg"], st["exp_avg_sq"]
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            lo = st.get("master_lo")
            pf = p.float() if lo is None else join_master(p, lo)
            pf.mul_(1.0 - group["lr"] * group["weight_decay"])
            denom = (v / bc2).sqrt_().add_(group["eps"])
            pf.addcdiv_(m / bc1, denom, value=-group["lr"])
            if lo is None:
                p.copy_(pf.to(p.dtype))
            else:
                hi, new_lo = split_master(pf)
                p.copy_(hi)
                lo.copy_(new_lo)

    def load_state_dict(self, state_dict):
        """Restore WITHOUT the base-class dtype cast: torch's
        Optimizer.load_state_dict casts fp state to the param dtype, which
        would silently truncate our fp32 moments to bf16 on bf16 params and
        break bitwise resume (tests/test_trainer_cpu.py
        test_resume_loss_continuity caught this).

        master_lo is restored as int16.  A saved state without it, loaded
        into a master-weight optimizer, starts from zeros (first touch); a
        saved state with it, loaded into an optimizer without the option,
        drops it and logs one line."""
        groups = self.param_groups
        saved_groups = state_dict["param_groups"]
        if len(groups) != len(saved_groups):
            raise ValueError("loaded state dict has a different number of "
                             "parameter groups")
        id_map = {
            old_id: p
            for old_g, g in zip(saved_groups, groups)
            for old_id, p in zip(old_g["params"], g["params"])
        }
        dropped = 0
        for k, v in state_dict["state"].items():
            p = id_map[k]
            self.state[p] = {
                "exp_avg": v["exp_avg"].to(device=p.device,
                                           dtype=torch.float32),
                "exp_avg_sq": v["exp_avg_sq"].to(device=p.device,
                                                 dtype=torch.float32),
            }
            lo = v.get("master_lo")
            if lo is None:
                continue
            if self.master_weights and p.dtype == torch.bfloat16:
                if lo.dtype != torch.int16 or lo.shape != p.shape:
                    raise ValueError(
                        "saved master_lo must be int16 of the parameter's "
                        f"shape, got {lo.dtype} {tuple(lo.shape)}")
                # clone: never alias the caller's tensor, the step writes it
                self.state[p]["master_lo"] = lo.to(
                    device=p.device).contiguous().clone()
            else:
                dropped += 1
        if dropped:
            LOGGER.warning(
                f"FusedAdamW: dropped the saved master_lo of {dropped} "
                "parameters (master_weights is off); the bf16 parameters "
                "are kept as they are")
        for g, saved in zip(groups, saved_groups):
            for key in saved:
                # max_grad_norm is this run's configuration, not training
                # state: the constructor's value holds across a resume
                if key not in ("params", "max_grad_norm"):
                    g[key] = saved[key]
        self._desc_cache.clear()  # state tensors were replaced
