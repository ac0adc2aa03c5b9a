"""Fused Adam over the flat arena.

A drop-in ``torch.optim.Optimizer`` (so ``LambdaLR`` / ``ReduceLROnPlateau``
drive it through ``param_groups[i]["lr"]``) whose ``step()`` is ONE HIP launch
over every parameter (``pbx_adam_flat``; ``pbx_adam_flat_groups`` with more
than one parameter group or AdamW's decoupled weight decay).  Its
``state_dict()`` has exactly the format of ``torch.optim.Adam`` so
reference-style checkpoints (``optimizer_state_dict``,
``ProteinBERT/utils.py:327-335``) load either way.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import torch

from .arena import ALIGN, FlatArena


def _hip_ok(t: torch.Tensor) -> bool:
    if t.device.type != "cuda":
        return False
    from ..ops import _lib
    if not _lib.available():
        raise _lib.HipError("GPU run but the HIP kernel library is not built; run ops.build")
    return True


MAX_GROUPS = 16       # PBX_ADAM_MAX_GROUPS of csrc/optim.hip


class FusedAdam(torch.optim.Optimizer):
    """``params``: a parameter list, a :class:`FlatArena`, or a list of group dicts as ``torch.optim.Adam``
    takes them.  ``lr``, ``betas``, ``eps``, ``weight_decay`` and ``decoupled_weight_decay`` (AdamW's rule)
    are per group; ``grad_scale``, the step counter and the skip flag are per optimizer.  The groups are
    fixed at construction: one byte per 64-element arena block names the block's group, and the update stays
    one launch (``pbx_adam_flat_groups``) whatever their number (at most 16)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, arena: Optional[FlatArena] = None, bf16_shadow: Optional[bool] = None,
                 decoupled_weight_decay: bool = False):
        if isinstance(params, FlatArena):
            arena, params = params, params.params
        params = list(params)
        if params and isinstance(params[0], dict):
            params = [{**g, "params": [p for p in g["params"] if p.requires_grad]} for g in params]
            if len(params) > MAX_GROUPS:
                raise ValueError(f"FusedAdam supports at most {MAX_GROUPS} param groups, got {len(params)}")
        else:
            params = [p for p in params if p.requires_grad]
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        self._groups_frozen = False
        super().__init__(params, defaults)
        self._groups_frozen = True
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam does not implement amsgrad / maximize")
            g["betas"] = tuple(g["betas"])
        grouped = [p for g in self.param_groups for p in g["params"]]
        self.arena = arena if arena is not None else FlatArena(grouped)
        a = self.arena
        self.exp_avg = torch.zeros_like(a.data)
        self.exp_avg_sq = torch.zeros_like(a.data)
        if bf16_shadow is None:   # default: keep a bf16 weight mirror whenever the arena is on the GPU
            bf16_shadow = a.data.is_cuda
        self.shadow = a.data.to(torch.bfloat16) if bf16_shadow else None
        if self.shadow is not None:
            a.attach_bf16_shadow(self.shadow)
        self.step_count = 0
        self.grad_scale = 1.0   # set to 1/world by the DP wrapper (SUM all-reduce -> mean)
        self.skip_flag: Optional[torch.Tensor] = None  # device int32; non-zero -> skip update
        dev = a.data.device
        # device-resident hyper-parameters + step counter: the update launch reads everything from
        # device memory, so it can be captured in a hipGraph and replayed; the host only rewrites
        # the hyper-parameter block when lr/betas/... change (prepare(), never during capture)
        G = len(self.param_groups)
        self._hp_dev = torch.zeros(8 * G, dtype=torch.float32, device=dev)   # [G][8], AdamHParams per group
        self._step_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._hp_host = None
        index = a.param_index()
        self._index = {}
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) not in index:
                    raise ValueError("a grouped parameter is not in the arena")
                self._index[id(p)] = index[id(p)]
        # group of every 64-element block, built once from the arena offsets; a segment's padding belongs to
        # its parameter's group.  _group_segs: each group's (offset, numel) segments in arena order (CPU path)
        table = torch.zeros(a.numel // ALIGN, dtype=torch.uint8)
        self._group_segs = []
        for gi, g in enumerate(self.param_groups):
            segs = sorted(a.segment(self._index[id(p)]) for p in g["params"])
            for o, n in segs:
                table[o // ALIGN:(o + n + ALIGN - 1) // ALIGN] = gi
            self._group_segs.append(segs)
        if G > 1 and len(self._index) != len(a.params):
            raise ValueError("with more than one group every arena parameter must be in a group")
        self._block_group = table.to(dev)

    # ---------------------------------------------------------------------------------
    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        if getattr(self, "_groups_frozen", False):
            raise ValueError("FusedAdam: the groups are fixed at construction (the arena's block table)")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = False) -> None:  # noqa: ARG002 - arena grads are views
        self.arena.zero_grad()

    def _hparam_values(self, group: int = 0):
        g = self.param_groups[group]
        b1, b2 = g["betas"]
        t = max(1, self.step_count)
        return (float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]),
                1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), float(self.grad_scale))

    def _decoupled_mask(self) -> int:
        return sum(1 << i for i, g in enumerate(self.param_groups) if g.get("decoupled_weight_decay"))

    def prepare(self) -> None:
        """Push changed hyper-parameters (any group's lr from a scheduler, grad scale) to the device block.
        Host -> device copy: call outside graph capture (the captured step reads the block)."""
        vals, key = (), ()
        for i in range(len(self.param_groups)):
            v = self._hparam_values(i)
            vals += v
            key += v[:5] + v[7:]
        if key != self._hp_host:
            self._hp_dev.copy_(torch.tensor(vals, dtype=torch.float32))
            self._hp_host = key

    def sync_step_counter(self) -> None:
        self._step_dev.fill_(float(self.step_count))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.begin_step()
        self.step_range(0, self.arena.numel)
        return loss

    @torch.no_grad()
    def begin_step(self) -> None:
        """Advance the step counters once per optimizer step; the update itself is one or more
        :meth:`step_range` launches (the DP path updates gradient buckets as their all-reduce lands)."""
        self.step_count += 1
        a = self.arena
        if not a.grads_attached():
            a.attach_grads()
        if _hip_ok(a.data):
            if not torch.cuda.is_current_stream_capturing():
                self.prepare()
            from ..ops import _lib
            _lib.call("pbx_add_scalar", self._step_dev.data_ptr(), 1.0, _lib.stream_ptr(self._step_dev.device))

    @torch.no_grad()
    def step_range(self, start: int, end: int) -> None:
        """Adam on arena elements ``[start, end)`` (element-wise, so any split of the arena gives the
        bitwise result of one whole-arena launch); ``start`` is a segment boundary (16-B aligned)."""
        a = self.arena
        if end <= start:
            return
        if _hip_ok(a.data):
            f4, b2 = 4 * start, 2 * start
            self._launch(a.data.data_ptr() + f4, a.grad.data_ptr() + f4, self.exp_avg.data_ptr() + f4,
                         self.exp_avg_sq.data_ptr() + f4, None if self.shadow is None else self.shadow.data_ptr() + b2,
                         start, end - start)
        else:
            if skip_requested(self.skip_flag):
                return
            sl = slice(start, end)
            self._update_host(start, end, a.data[sl], a.grad[sl], self.exp_avg[sl], self.exp_avg_sq[sl])
            if self.shadow is not None:
                self.shadow[sl].copy_(a.data[sl])

    def _launch(self, p: int, g: int, m: int, v: int, shadow: Optional[int], start: int, n: int) -> None:
        """The update launch on ``n`` elements whose first is arena element ``start`` (a multiple of 64).
        One group without decoupled decay is ``pbx_adam_flat``; anything else is ``pbx_adam_flat_groups``
        with the block table advanced by ``start / 64``."""
        from ..ops import _lib
        dev = self.arena.data.device
        mask = self._decoupled_mask()
        G = len(self.param_groups)
        if G == 1 and mask == 0:
            _lib.call("pbx_adam_flat", p, g, m, v, shadow, n, self._hp_dev.data_ptr(), _lib.ptr(self.skip_flag),
                      self._step_dev.data_ptr(), _lib.stream_ptr(dev))
            return
        if start % ALIGN:
            raise ValueError(f"a grouped update starts on a {ALIGN}-element boundary, got {start}")
        _lib.call("pbx_adam_flat_groups", p, g, m, v, shadow, n, self._hp_dev.data_ptr(), G, mask,
                  self._block_group.data_ptr() + start // ALIGN, _lib.ptr(self.skip_flag),
                  self._step_dev.data_ptr(), _lib.stream_ptr(dev))

    def _update_host(self, start: int, end: int, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                     v: torch.Tensor) -> None:
        """CPU update of arena elements ``[start, end)``; the flat tensors hold exactly that range."""
        if len(self.param_groups) == 1 and self._decoupled_mask() == 0:
            adam_update_host(self, p, g, m, v)
        else:
            adam_update_host_groups(self, start, end, p, g, m, v)

    @torch.no_grad()
    def set_nonfinite_skip(self) -> torch.Tensor:
        """Device flag (int32 [1]): 1 when any arena gradient is NaN / Inf; the update then leaves
        parameters and moments unchanged.  No host sync (two HIP launches on a GPU)."""
        a = self.arena
        if _hip_ok(a.grad):
            from ..ops import _lib
            if getattr(self, "_nf_ws", None) is None:
                self._nf_ws = torch.empty(1025, dtype=torch.int32, device=a.grad.device)
            _lib.call("pbx_nonfinite_flag", a.grad.data_ptr(), a.numel, self._nf_ws.data_ptr(),
                      self._nf_ws[1024:].data_ptr(), float("inf"), 0, _lib.stream_ptr(a.grad.device))
            self.skip_flag = self._nf_ws[1024:]
        else:
            # exact per-element test in one BLAS pass: grad . 0 is NaN iff some element is NaN / Inf (every
            # finite product is exactly 0, so large finite gradients cannot overflow it, unlike a sum)
            z = getattr(self, "_zero_vec", None)
            if z is None or z.numel() != a.grad.numel() or z.dtype != a.grad.dtype:
                z = self._zero_vec = torch.zeros_like(a.grad)
            bad = not bool(torch.isfinite(torch.dot(a.grad, z)))
            self.skip_flag = torch.tensor([1 if bad else 0], dtype=torch.int32)
        return self.skip_flag

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Global L2 grad-norm clip over the arena (after DP reduction); returns the pre-clip norm."""
        a = self.arena
        if _hip_ok(a.grad):
            from ..ops import _lib
            ws = torch.empty(1025, dtype=torch.float32, device=a.grad.device)
            _lib.call("pbx_sumsq_flat", a.grad.data_ptr(), a.numel, ws.data_ptr(), ws[1024:].data_ptr(),
                      _lib.stream_ptr(a.grad.device))
            # sumsq of the (grad_scale-scaled) mean gradient: the clip coefficient max_norm / norm
            # is scale-invariant once both sides refer to the same gradient, so the raw threshold
            # is passed (the coefficient multiplies the unscaled SUM gradient in place)
            sumsq = ws[1024:] * (self.grad_scale ** 2)
            _lib.call("pbx_clip_scale_flat", a.grad.data_ptr(), a.numel, sumsq.data_ptr(),
                      float(max_norm), _lib.stream_ptr(a.grad.device))
            return sumsq.sqrt()[0]
        norm = (a.grad * self.grad_scale).norm()
        c = max_norm / (norm + 1e-6)
        if c < 1:
            a.grad.mul_(c)
        return norm

    # ---------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """``torch.optim.Adam``'s format: parameter ids numbered consecutively across the groups, one
        ``param_groups`` entry per group."""
        state, groups, i = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                if self.step_count > 0:
                    o, n = self.arena.segment(self._index[id(p)])
                    state[i] = {"step": torch.tensor(float(self.step_count)),
                                "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                                "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
                ids.append(i)
                i += 1
            group = {k: v for k, v in g.items() if k != "params"}
            group["params"] = ids
            groups.append(group)
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or \
                any(len(s["params"]) != len(g["params"]) for s, g in zip(groups, self.param_groups)):
            raise ValueError("optimizer state does not match the parameter groups")
        st = state_dict["state"]
        steps, i = 0, 0
        for saved, g in zip(groups, self.param_groups):
            for k, v in saved.items():
                if k != "params":
                    g[k] = tuple(v) if k == "betas" else v
            for p in g["params"]:
                s = st[i] if i in st else st.get(str(i))
                i += 1
                if s is None:
                    continue
                o, n = self.arena.segment(self._index[id(p)])
                self.exp_avg[o:o + n].copy_(s["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(s["exp_avg_sq"].reshape(-1))
                steps = int(float(s["step"]))
        self.step_count = steps
        self.sync_step_counter()


def skip_requested(flag: Optional[torch.Tensor]) -> bool:
    return flag is not None and bool(flag.reshape(-1)[0].item())


def adam_update_host(opt: FusedAdam, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor) -> None:
    """In-place Adam on flat host tensors with ``opt``'s hyper-parameters (torch's fused CPU kernel)."""
    lr, b1, b2, eps, wd, _, _, gs = opt._hparam_values()
    grad = g if gs == 1.0 else g * gs
    if getattr(opt, "_host_step", None) is None:
        opt._host_step = torch.zeros((), dtype=torch.float32)
    opt._host_step.fill_(float(max(1, opt.step_count)))
    torch._fused_adam_([p], [grad], [m], [v], [], [opt._host_step], amsgrad=False, lr=lr, beta1=b1, beta2=b2,
                       weight_decay=wd, eps=eps, maximize=False)


def adam_update_host_groups(opt: FusedAdam, start: int, end: int, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                            v: torch.Tensor) -> None:
    """In-place Adam / AdamW on flat host tensors that hold arena elements ``[start, end)``: torch's fused CPU
    kernel once per group, over the parts of that group's segments inside the range."""
    if getattr(opt, "_host_step", None) is None:
        opt._host_step = torch.zeros((), dtype=torch.float32)
    opt._host_step.fill_(float(max(1, opt.step_count)))
    for gi, group in enumerate(opt.param_groups):
        cuts = [(max(o, start) - start, min(o + n, end) - start) for o, n in opt._group_segs[gi]
                if o < end and o + n > start]
        if not cuts:
            continue
        lr, b1, b2, eps, wd, _, _, gs = opt._hparam_values(gi)
        grads = [g[a:b] if gs == 1.0 else g[a:b] * gs for a, b in cuts]
        fused = torch._fused_adamw_ if group.get("decoupled_weight_decay") else torch._fused_adam_
        fused([p[a:b] for a, b in cuts], grads, [m[a:b] for a, b in cuts], [v[a:b] for a, b in cuts], [],
              [opt._host_step] * len(cuts), amsgrad=False, lr=lr, beta1=b1, beta2=b2, weight_decay=wd, eps=eps,
              maximize=False)


def param_groups_for(model: torch.nn.Module, lr: float, weight_decay: float = 0.0, no_decay=("bias", "norm"),
                     lr_scale: Optional[Dict[str, float]] = None):
    """Group dicts for :class:`FusedAdam` / ``torch.optim.Adam``: the trainable parameters whose name contains
    one of the ``no_decay`` substrings get ``weight_decay = 0``; ``lr_scale`` maps a name prefix to a factor on
    ``lr`` (the longest matching prefix counts), e.g. ``{"encoder.": 0.1}``.  One group per (factor, decays)
    pair that occurs, in the order of its first parameter in ``model.named_parameters()``."""
    prefixes = sorted((lr_scale or {}).items(), key=lambda kv: (-len(kv[0]), kv[0]))
    no_decay = tuple(no_decay or ())
    groups: Dict[Any, Dict[str, Any]] = {}
    seen = set()
    for name, p in model.named_parameters():
        if not p.requires_grad or id(p) in seen:
            continue
        seen.add(id(p))
        scale = next((float(f) for pre, f in prefixes if name.startswith(pre)), 1.0)
        decays = weight_decay != 0.0 and not any(s in name for s in no_decay)
        key = (scale, decays)
        if key not in groups:
            groups[key] = {"params": [], "lr": lr * scale, "weight_decay": weight_decay if decays else 0.0}
        groups[key]["params"].append(p)
    return list(groups.values())


def make_optimizer(model: torch.nn.Module, lr: float = 2e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                   weight_decay: float = 0.0, arena: Optional[FlatArena] = None, groups=None,
                   decoupled_weight_decay: bool = False) -> FusedAdam:
    """``groups``: group dicts over ``model``'s parameters (:func:`param_groups_for`).  The arena is still
    built from ``model.parameters()``, so its reverse-registration layout (the DP buckets rely on it) does not
    depend on the grouping."""
    if groups is not None:
        arena = arena if arena is not None else FlatArena(model.parameters())
        return FusedAdam(groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, arena=arena,
                         decoupled_weight_decay=decoupled_weight_decay)
    return FusedAdam(model.parameters() if arena is None else arena.params, lr=lr, betas=betas, eps=eps,
                     weight_decay=weight_decay, arena=arena, decoupled_weight_decay=decoupled_weight_decay)
