"""Per-residue fine-tuning head on MI355X (BASELINE cfg 5).

``logits = h Wᵀ + b`` over ``[B*L, 128]`` bf16 encoder rows and K <= 16 classes.  The head weight
stays an fp32 parameter and the logits keep fp32 accuracy: one streaming kernel (``csrc/finetune.hip``
``token_head_fwd``, a thread per residue, W broadcast from LDS) runs fp32 FMAs over the exact bf16
rows -- the fp32 ``F.linear`` result on an upcast copy, memory-bound on the 67 MB row read at
B*L = 262,144 (round 3-4 used two library bf16 GEMMs on a hi / lo weight split, 2 x 25 us).  The weight gradient, a 262,144-long reduction that hipBLASLt ran at 230-410 us,
is the streaming kernel in ``csrc/finetune.hip`` (fp32 accumulation, deterministic slab reduction);
the input gradient (unfrozen encoders only) is fp32.

``hidden="all"`` heads read every block's hidden state: :class:`MultiTokenHeadFn` is the same pair of
kernels over up to 8 row sources (``token_head_multi_fwd`` / ``token_head_multi_wgrad``), so the
concatenated ``[B*L, nb*128]`` feature matrix (and its fp32 copy) is never written.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from . import _lib

MAX_SOURCES = 8


def supported(h: torch.Tensor, n_classes: int) -> bool:
    return h.is_cuda and h.dtype == torch.bfloat16 and h.shape[-1] == 128 and n_classes <= 16


class TokenHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias):
        B, L, C = h.shape
        h2 = h.contiguous().view(B * L, C)
        K = weight.shape[0]
        # one streaming pass: fp32 FMAs over the exact bf16 rows and fp32 weights (csrc/finetune.hip)
        logits = torch.empty((B * L, K), dtype=torch.float32, device=h.device)
        _lib.call("pbx_token_head_fwd", h2.data_ptr(), weight.detach().float().contiguous().data_ptr(),
                  bias.detach().float().contiguous().data_ptr(), logits.data_ptr(), B * L, K,
                  _lib.stream_ptr(h.device))
        ctx.save_for_backward(h2, weight)
        ctx.shape = (B, L)
        return logits.view(B, L, -1)

    @staticmethod
    def backward(ctx, dlogits):
        h2, weight = ctx.saved_tensors
        B, L = ctx.shape
        K = weight.shape[0]
        g = dlogits.reshape(B * L, K).float().contiguous()
        dh = dw = db = None
        if ctx.needs_input_grad[0]:
            dh = torch.mm(g, weight.float()).view(B, L, -1).to(h2.dtype)
        if ctx.needs_input_grad[1]:
            M = B * L
            P = max(1, min(2 * torch.cuda.get_device_properties(h2.device).multi_processor_count, (M + 15) // 16))
            slab = torch.empty((P, K, h2.shape[1]), dtype=torch.float32, device=h2.device)
            st = _lib.stream_ptr(h2.device)
            _lib.call("pbx_token_head_wgrad", h2.data_ptr(), g.data_ptr(), slab.data_ptr(), M, K, P, st)
            dw = torch.zeros_like(weight)
            _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * h2.shape[1], dw.data_ptr(), None, st)
        if ctx.needs_input_grad[2]:
            db = g.sum(dim=0)
        return dh, dw, db


def supported_multi(hs: Sequence[torch.Tensor], n_classes: int) -> bool:
    """The fused all-block head: 1..8 CUDA bf16 ``[B, L, 128]`` sources of one shape and K <= 16."""
    if not 1 <= len(hs) <= MAX_SOURCES or not 1 <= n_classes <= 16:
        return False
    h0 = hs[0]
    return all(h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and h.shape[-1] == 128
               and h.shape == h0.shape and h.device == h0.device for h in hs)


def multi_head_torch(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                     gterm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition on any device: ``Linear(cat_i h_i) + gterm`` broadcast over L, in fp32."""
    logits = torch.nn.functional.linear(torch.cat([h.float() for h in hs], dim=-1), weight, bias)
    return logits if gterm is None else logits + gterm.unsqueeze(1)


def _rows(h: torch.Tensor) -> torch.Tensor:
    """``[B, L, 128]`` as row-contiguous, 16-byte aligned ``[B*L, 128]`` (a copy only when it is not already)."""
    h2 = h.contiguous().view(-1, h.shape[-1])
    return h2 if h2.data_ptr() % 16 == 0 else h2.clone()


def _src_array(rows: List[torch.Tensor]):
    """Host array of the sources' device addresses (the launcher copies it into the kernel's arguments)."""
    return (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])


def wgrad_slab_rows(M: int, device) -> int:
    return max(1, min(2 * torch.cuda.get_device_properties(device).multi_processor_count, (M + 15) // 16))


class MultiTokenHeadFn(torch.autograd.Function):
    """``apply(h_0, ..., h_{nb-1}, weight [K, nb*128], bias [K], gterm [B, K] | None)`` -> logits ``[B, L, K]``:
    ``bias + sum_i h_i @ weight[:, i*128:(i+1)*128].T + gterm`` broadcast over L, fp32 FMAs over the exact bf16
    rows, blocks in ascending order."""

    @staticmethod
    def forward(ctx, *args):
        hs, (weight, bias, gterm) = args[:-3], args[-3:]
        nb = len(hs)
        B, L, C = hs[0].shape
        K = weight.shape[0]
        if weight.shape[1] != nb * C:
            raise ValueError(f"weight {tuple(weight.shape)} for {nb} sources of {C} channels")
        M = B * L
        rows = [_rows(h) for h in hs]
        gt = None if gterm is None else gterm.detach().float().contiguous()
        if gt is not None and tuple(gt.shape) != (B, K):
            raise ValueError(f"gterm {tuple(gt.shape)}: expected {(B, K)}")
        w32 = weight.detach().float().contiguous()
        b32 = bias.detach().float().contiguous()
        logits = torch.empty((M, K), dtype=torch.float32, device=hs[0].device)
        _lib.call("pbx_token_head_multi_fwd", _src_array(rows), nb, w32.data_ptr(), b32.data_ptr(), _lib.ptr(gt),
                  logits.data_ptr(), M, K, L, _lib.stream_ptr(hs[0].device))
        ctx.save_for_backward(weight, *rows)
        ctx.shape = (B, L, nb)
        ctx.has_gterm = gterm is not None
        return logits.view(B, L, K)

    @staticmethod
    def backward(ctx, dlogits):
        weight, *rows = ctx.saved_tensors
        B, L, nb = ctx.shape
        K, C = weight.shape[0], rows[0].shape[1]
        M = B * L
        g = dlogits.reshape(M, K).float().contiguous()
        dhs = [None] * nb
        if any(ctx.needs_input_grad[:nb]):
            w32 = weight.float()
            for i in range(nb):
                if ctx.needs_input_grad[i]:
                    dhs[i] = torch.mm(g, w32[:, i * C:(i + 1) * C]).view(B, L, C).to(rows[i].dtype)
        dw = db = dgt = None
        if ctx.needs_input_grad[nb]:
            dev = rows[0].device
            P = wgrad_slab_rows(M, dev)
            slab = torch.empty((P, K, nb * C), dtype=torch.float32, device=dev)
            st = _lib.stream_ptr(dev)
            _lib.call("pbx_token_head_multi_wgrad", _src_array(rows), nb, g.data_ptr(), slab.data_ptr(), M, K, P, st)
            dw = torch.zeros_like(weight)
            _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * nb * C, dw.data_ptr(), None, st)
        if ctx.needs_input_grad[nb + 1]:
            db = g.sum(dim=0)
        if ctx.has_gterm and ctx.needs_input_grad[nb + 2]:
            dgt = g.view(B, L, K).sum(dim=1)
        return (*dhs, dw, db, dgt)
